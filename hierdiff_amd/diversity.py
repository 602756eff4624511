"""Diverse sampling: the rows of a group repel each other by their aligned RMSD inside the path loop (particle guidance) - host side
(the `Diversity` keyword, the group checks, the per-transition rows, the result entries) and the float64 torch form of the potential.

A diverse call runs P rows per group: the batch is B = G * P rows, group g owns rows g P .. g P + P - 1 (the layout of
hierdiff_amd/steering.py).  At every transition, behind the network call, guidance and the restraint updates of eps^, the data
predictions x^0 of a group's rows are compared pair by pair after optimal rigid superposition (a proper rotation: mirror images stay
apart), over the nodes A valid in both rows (n = |A|):

    d2_pq = min_R sum_A |(x_p - c_p) - R (x_q - c_q)|^2 / n,    Phi = strength * sum_{p<q} exp(-d2_pq / (2 length^2))

and eps^_x += project(clip(s_g lambda_k dPhi/dx)) - the update of `restraints=` with Phi in the place of U, so x^0 moves down Phi and
the rows move apart (hd_set_diversity / hd_diversity_attach / k_diverse.hpp, include/hierdiff_hip.h).  The gradient needs no dR/dx:
R maximises the overlap, so dPhi/dx_p,i = -(strength / (length^2 n)) sum_q e_pq r_i with the residual r under the best fit.  Unlike
steering it is a gradient, not a selection: it also acts on the deterministic paths (eta = 0, solver "dpm2m") and needs no restraints.

THE CONTRACT.  A group's result depends on the seed, the ids of its rows, P, its masks, contexts and tables, the weights, the schedule
and the path only - not on the other groups of the batch, on where the batch was cut (at group boundaries), on graph replay versus
plain launches, or on how `path_steps` cuts the chain.  Rows of a group interact; groups do not.  No state crosses transitions.

Mechanism only: which length and strength help is for a trained checkpoint to show."""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import numpy as np
import torch

MAX_PARTICLES = 32
WHERE = "sample / sample_from_masks / path_steps / sample_from_latent / latent_steps / vary"
SCHEDULES = ("score", "sigma")


def _is_int(v) -> bool:
    return not isinstance(v, bool) and isinstance(v, (int, np.integer))


def _is_num(v) -> bool:
    return not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating))


class Diversity:
    """The `diversity=` keyword of the sampling entry points.

    particles   P, rows per group (1: the keyword does nothing); at most 32
    length      l > 0, the width of the Gaussian in the units of the aligned RMSD (data units)
    strength    kappa >= 0 (0: the keyword does nothing)
    scale       a number, or one per group [G] (all 0: the keyword does nothing); a group with scale 0 is left alone
    schedule    lambda_k: "score" (nv0 sigma_t / alpha_t), "sigma", or K explicit weights - `restraints.lambda_rows`
    clip        the largest step per node in eps units (None: no clip)"""

    def __init__(self, particles, length, strength=1.0, scale=1.0, schedule="score", clip=None):
        from .restraints import check_clip
        if not _is_int(particles) or int(particles) < 1:
            raise ValueError(f"Diversity: particles must be an integer >= 1, got {particles!r}")
        if int(particles) > MAX_PARTICLES:
            raise ValueError(f"Diversity: particles must be <= {MAX_PARTICLES} (one workgroup holds a group's pairs), got {particles}")
        if not _is_num(length) or not math.isfinite(float(length)) or not float(length) > 0.0:
            raise ValueError(f"Diversity: length must be a finite number > 0, got {length!r}")
        if not _is_num(strength) or not math.isfinite(float(strength)) or float(strength) < 0.0:
            raise ValueError(f"Diversity: strength must be a finite number >= 0, got {strength!r}")
        if isinstance(scale, bool):
            raise ValueError(f"Diversity: scale must be a number or a [G] tensor, got {scale!r}")
        try:
            s = torch.as_tensor(scale, dtype=torch.float32).detach().cpu()
        except (TypeError, ValueError, RuntimeError):
            raise ValueError(f"Diversity: scale must be a number or a [G] tensor, got {scale!r}") from None
        s = s.reshape(1) if s.dim() == 0 else s
        if s.dim() != 1 or s.numel() < 1 or not bool(torch.isfinite(s).all()):
            raise ValueError("Diversity: scale must be a finite number or a [G] tensor")
        if isinstance(schedule, str):
            if schedule not in SCHEDULES:
                raise ValueError(f"Diversity: schedule must be one of {SCHEDULES} or a length-K sequence, got {schedule!r}")
        else:
            try:
                schedule = tuple(float(v) for v in torch.as_tensor(schedule, dtype=torch.float64).reshape(-1).tolist())
            except (TypeError, ValueError, RuntimeError):
                raise ValueError(f"Diversity: schedule must be one of {SCHEDULES} or a length-K sequence, got {schedule!r}") from None
            if not schedule or not all(math.isfinite(v) for v in schedule):
                raise ValueError("Diversity: an explicit schedule holds one finite weight per transition")
        try:
            self.clip = check_clip(clip)
        except ValueError:
            raise ValueError(f"Diversity: clip must be a positive number (None or inf: no clip), got {clip!r}") from None
        self.P, self.length, self.strength = int(particles), float(length), float(strength)
        self.scale, self.schedule = s.contiguous(), schedule

    @property
    def active(self) -> bool:
        """False: the call runs the code path without the keyword, untouched."""
        return self.P > 1 and self.strength != 0.0 and bool((self.scale != 0).any())

    def key(self):
        return (self.schedule, self.clip)

    def slice(self, lo: int, hi: int) -> "Diversity":
        """The keyword of groups lo .. hi-1 (a batch of the list-level calls)."""
        if self.scale.numel() == 1:
            return self
        import copy
        d = copy.copy(self)
        d.scale = self.scale[lo:hi].contiguous()
        return d

    def __repr__(self):
        return (f"Diversity(particles={self.P}, length={self.length}, strength={self.strength}, scale={self.scale.tolist()}, "
                f"schedule={self.schedule!r}, clip={self.clip})")

    def energy(self, x: torch.Tensor, node_mask: torch.Tensor, model=None):
        """(Phi [G], rmsd [G, P, P]) float64 of positions x [B, N, 3] in data units under node_mask [B, N, 1]: on a device the HIP
        kernel (k_diverse_energy; `model`: the DiffusionQM9 that owns the library handle), on the CPU the same formulas in torch
        float64.  The matrix is symmetric with a zero diagonal; a pair that contributes nothing (at most one common valid node, a
        non-finite coordinate) is NaN."""
        B, N = _batch_shape(x, node_mask)
        if B % self.P:
            raise ValueError(f"Diversity.energy: the batch ({B}) must be a multiple of particles ({self.P})")
        if self.P < 2:
            raise ValueError("Diversity.energy: needs particles >= 2")
        if x.device.type != "cuda":
            return energy_terms(x.detach().double(), node_mask, self.P, self.length, self.strength, return_rmsd=True)
        return _device_energy(x, node_mask, self.P, self.length, self.strength, model, "Diversity.energy")


def _batch_shape(x, node_mask):
    B, N = int(node_mask.shape[0]), int(node_mask.shape[1])
    if tuple(x.shape) != (B, N, 3):
        raise ValueError(f"x must be [{B}, {N}, 3], got {tuple(x.shape)}")
    return B, N


def _device_energy(x, node_mask, P: int, length: float, strength: float, model, what: str, _attach=None):
    """(`_attach`: the scales and nv0 of the sampling call whose result this is - the energy reads neither, and attaching what the
    call attached keeps its cached graph.)"""
    if model is None:
        raise ValueError(f"{what} on a device needs model= (the DiffusionQM9 that owns the library handle)")
    from . import _lib
    from .dynamics import _stream
    dev = x.device
    B, N = int(node_mask.shape[0]), int(node_mask.shape[1])
    h, stream = model._lib_handle(), _stream(dev)
    topo = model.dynamics.topology(node_mask.to(dev), None, B, N)
    xs = x.detach().to(torch.float32).contiguous()
    scale, nv0 = (torch.ones(1), 1.0) if _attach is None else _attach
    lib = _lib.load()
    attach(topo, P, strength, length, scale, nv0, stream)
    try:
        phi = torch.empty(B // P, device=dev, dtype=torch.float64)
        rmsd = torch.empty((B // P, P, P), device=dev, dtype=torch.float64)
        _lib.check(lib.hd_diversity_energy(h, topo.ptr, xs.data_ptr(), phi.data_ptr(), rmsd.data_ptr(), stream), "hd_diversity_energy")
        return phi, rmsd
    finally:
        _lib.check(lib.hd_diversity_detach(topo.ptr), "hd_diversity_detach")


def attach(topo, P: int, strength: float, length: float, scale, nv0: float, stream) -> None:
    """Attach diversity to `topo` (hd_diversity_attach): P rows per group, kappa, l, the per-group scales (host values) and nv0."""
    import ctypes as C
    from . import _lib
    sc = np.ascontiguousarray(torch.as_tensor(scale, dtype=torch.float32).reshape(-1).numpy())
    _lib.check(_lib.load().hd_diversity_attach(topo.ptr, int(P), float(strength), float(length), sc.ctypes.data_as(C.POINTER(C.c_float)),
                                               int(sc.shape[0]), float(nv0), stream), "hd_diversity_attach")


def kabsch_rotation(S: torch.Tensor) -> torch.Tensor:
    """R [3, 3] = argmax over proper rotations of tr(R^T S) for S = sum x' y'^T (x' ~ R y'): S = U diag(s) V^T, R = U diag(1, 1,
    det(U V^T)) V^T - the determinant fix keeps a reflection out."""
    U, _, Vh = torch.linalg.svd(S)
    d = torch.sign(torch.linalg.det(U @ Vh))
    d = torch.where(d == 0, torch.ones_like(d), d)
    return U @ torch.diag(torch.stack([torch.ones_like(d), torch.ones_like(d), d])) @ Vh


def energy_terms(x: torch.Tensor, node_mask: torch.Tensor, P: int, length: float, strength: float = 1.0, return_rmsd: bool = False):
    """Phi [G] in x's dtype, differentiable in x [B, N, 3]: the formulas of the module docstring in torch.  R is found under no_grad
    through `torch.linalg.svd` with the determinant fix - it maximises, so autograd through the rest gives the exact gradient.
    `return_rmsd`: (Phi, rmsd [G, P, P]) with the matrix detached, NaN for a pair that contributes nothing."""
    B, N = _batch_shape(x, node_mask)
    P = int(P)
    if P < 2 or B % P:
        raise ValueError(f"energy_terms: need particles >= 2 and a batch ({B}) that is a multiple of it, got {P}")
    nm = node_mask.reshape(B, N).bool().to(x.device)
    G = B // P
    rmsd = torch.full((G, P, P), float("nan"), dtype=x.dtype, device=x.device)
    phis = []
    for g in range(G):
        phi = x.new_zeros(())
        for p in range(P):
            rmsd[g, p, p] = 0.0
            for q in range(p + 1, P):
                a = nm[g * P + p] & nm[g * P + q]
                xp, xq = x[g * P + p][a], x[g * P + q][a]
                n = int(a.sum())
                if n <= 1 or not bool(torch.isfinite(xp).all() and torch.isfinite(xq).all()):
                    continue
                xp, xq = xp - xp.mean(0), xq - xq.mean(0)
                with torch.no_grad():
                    R = kabsch_rotation(xp.transpose(0, 1) @ xq)
                r = xp - xq @ R.transpose(0, 1)
                d2 = (r * r).sum() / n
                phi = phi + torch.exp(-d2 / (2.0 * length * length))
                rmsd[g, p, q] = rmsd[g, q, p] = torch.sqrt(d2.detach())
        phis.append(strength * phi)
    phi = torch.stack(phis)
    return (phi, rmsd) if return_rmsd else phi


def pairwise_rmsd(x: torch.Tensor, node_mask: torch.Tensor, P: int, model=None) -> torch.Tensor:
    """[G, P, P] float64, the aligned RMSD between the rows of every group of P rows of x [B, N, 3]: HIP on a device (`model` owns the
    handle), torch float64 on the CPU.  Symmetric, zero diagonal, NaN for a pair with at most one common valid node."""
    B, _ = _batch_shape(x, node_mask)
    if not _is_int(P) or int(P) < 2 or B % int(P):
        raise ValueError(f"pairwise_rmsd: need particles >= 2 and a batch ({B}) that is a multiple of it, got {P!r}")
    if int(P) > MAX_PARTICLES:
        raise ValueError(f"pairwise_rmsd: particles must be <= {MAX_PARTICLES}, got {P}")
    if x.device.type != "cuda":
        return energy_terms(x.detach().double(), node_mask, int(P), 1.0, 1.0, return_rmsd=True)[1]
    return _device_energy(x, node_mask, int(P), 1.0, 1.0, model, "pairwise_rmsd")[1]


def wanted(model, diversity=None) -> bool:
    """Whether the keyword (None: the model's `diversity`) asks for the update at all.  None, particles = 1, or a strength or scale of
    0 is the code path without it; anything else - a value that is no `Diversity` included, which `resolve` then refuses - asks for it."""
    dv = getattr(model, "diversity", None) if diversity is None else diversity
    if dv is None:
        return False
    return dv.active if isinstance(dv, Diversity) else True


def resolve(model, diversity, eta, K: int, B: Optional[int] = None, what: str = "diversity", injected: bool = False,
            steered: bool = False) -> Optional[Diversity]:
    """Keyword (None: the model's `diversity`) -> None for the code path without it, untouched, or the `Diversity`.  `K`: the plan's
    transitions; `steered`: the plan steers.  Pure host checks."""
    if not wanted(model, diversity):
        return None
    dv = getattr(model, "diversity", None) if diversity is None else diversity
    if not isinstance(dv, Diversity):
        raise ValueError(f"{what}: diversity must be a hierdiff_amd.diversity.Diversity, got {type(dv).__name__}")
    if steered:
        raise NotImplementedError(f"{what}: diversity= and steering (particles=) in one call are not supported: both lay groups over "
                                  "the batch, and duplicated particles would be pushed apart again")
    if not isinstance(dv.schedule, str) and len(dv.schedule) != int(K):
        raise ValueError(f"{what}: the diversity schedule holds one finite weight per transition ({K}), got {len(dv.schedule)}")
    if B is not None:
        if int(B) % dv.P != 0:
            raise ValueError(f"{what}: the batch ({B}) must be a multiple of the diversity's particles ({dv.P}): group g owns rows "
                             "g P .. g P + P - 1")
        if dv.scale.numel() not in (1, int(B) // dv.P):
            raise ValueError(f"{what}: the diversity scale must hold one value per group ([{int(B) // dv.P}]), got {dv.scale.numel()}")
    return dv


def stochastic(eta) -> bool:
    """Whether the plan's update draws on the path: eta > 0, or solver "sde2m"."""
    if getattr(eta, "stochastic", None) is not None:
        return bool(eta.stochastic)
    return float(eta) != 0.0


def refuse(model, what: str, diversity=None, why: str = "") -> None:
    """Entry points that take no diversity: an error when the keyword or the model's attribute asks for it, instead of ignoring it."""
    if wanted(model, diversity):
        raise NotImplementedError(f"{what}: diverse sampling is not supported here{why} (the `diversity` keyword, or model.diversity); "
                                  f"it acts in {WHERE}")


def _rows_equal(t: torch.Tensor, P: int) -> bool:
    g = t.reshape(t.shape[0] // P, P, -1)
    return bool((g == g[:, :1]).all())


def check_groups(dv: Diversity, node_mask, context=None, what: str = "diversity") -> None:
    """All rows of a group must have equal node masks and context rows (as `steering.check_groups`).  Compared on the host."""
    P = dv.P
    nm = torch.as_tensor(node_mask).detach().cpu()
    B = int(nm.shape[0])
    if B % P != 0:
        raise ValueError(f"{what}: the batch ({B}) must be a multiple of the diversity's particles ({P}): group g owns rows "
                         "g P .. g P + P - 1")
    if dv.scale.numel() not in (1, B // P):
        raise ValueError(f"{what}: the diversity scale must hold one value per group ([{B // P}]), got {dv.scale.numel()}")
    bad = None
    if not _rows_equal(nm.reshape(B, -1), P):
        bad = "node masks"
    elif context is not None and not _rows_equal(torch.as_tensor(context).detach().cpu().reshape(B, -1), P):
        bad = "context rows"
    if bad is not None:
        raise ValueError(f"{what}: the {bad} differ inside a group of {P} rows (rows g P .. g P + P - 1 must be equal)")


def rows(gamma, path, dv: Diversity, nv0: float) -> np.ndarray:
    """[K, 4] float32 rows {alpha_t, sigma_t, lambda_k, clip_k} of the transitions of `path`: `restraints.lambda_rows`."""
    from .restraints import lambda_rows
    return lambda_rows(gamma, path, dv.schedule if isinstance(dv.schedule, str) else list(dv.schedule), dv.clip, nv0)


class Result(NamedTuple):
    """What a diverse call leaves as `model.diversity_last` (CPU tensors), evaluated on the returned x."""
    phi: torch.Tensor           # [G] float64
    mean_rmsd: torch.Tensor     # [G] float64: the mean over the pairs that contribute (NaN: none does)
    rmsd: torch.Tensor          # [G, P, P] float64
    group: torch.Tensor         # [B] int64


def result(phi: torch.Tensor, rmsd: torch.Tensor) -> Result:
    phi, rmsd = phi.detach().cpu(), rmsd.detach().cpu()
    G, P = int(rmsd.shape[0]), int(rmsd.shape[1])
    iu = torch.triu_indices(P, P, 1)
    pairs = rmsd[:, iu[0], iu[1]]
    ok = torch.isfinite(pairs)
    cnt = ok.sum(1)
    mean = torch.where(ok, pairs, torch.zeros_like(pairs)).sum(1) / cnt.clamp(min=1)
    mean = torch.where(cnt > 0, mean, torch.full_like(mean, float("nan")))
    return Result(phi, mean, rmsd, torch.arange(G * P) // P)


def into(results, res: Result, lo: int = 0, group0: int = 0) -> None:
    """'diversity_group' and 'diversity_rmsd' ([P] float64: the aligned RMSD of the returned x to every row of its group, own entry 0)
    into the dicts of rows lo .. lo + len(results) - 1 of `res`."""
    P = int(res.rmsd.shape[1])
    for i, r in enumerate(results):
        b = lo + i
        r['diversity_group'] = res.group[b] + group0
        r['diversity_rmsd'] = res.rmsd[b // P, b % P].clone()
