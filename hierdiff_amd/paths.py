"""Few-step sampling: paths through the trained time grid and their per-transition coefficient rows.

A path is a strictly decreasing list of grid indices T = t_0 > t_1 > ... > t_K = 0; transition k goes from t = t_k to
s = t_{k+1}.  The update of `sample_p_zs_given_zt` (diffusion_qm9.py:312-345) is written for any s < t, so a path needs no
retraining and no new network code - only rows of coefficients from the SAME gamma grid the plain schedule uses
(`noise_model.schedule_tables`), which `path_tables` computes on the host:

  eta = 1      ancestral rows {alpha_t|s, sigma2_t|s, sigma_t, sigma} = `step_coefficients(g[s], g[t])`: the plain loop's own row
               format, so the identity path T, T-1, .., 0 gives the plain table bit for bit;
  0 <= eta < 1 linear rows {a, b, c, 0} of z_s = a z_t - b eps + c noise with sigma~ = eta sigma_t|s sigma_s / sigma_t,
               a = alpha_s / alpha_t, b = alpha_s sigma_t / alpha_t - sqrt(sigma_s^2 - sigma~^2), c = sigma~ (the DDIM family;
               eta = 0 is the noise-free update), evaluated in float64 and rounded once.  At eta = 1 this is the ancestral update
               algebraically; the ancestral format is kept there so that stride 1 stays bit-identical.

  solver="dpm2m"  multistep rows {a, b, c2, p, q} (`multistep_coefficients`): the eta = 0 row plus one correction from the previous
               transition's data prediction, z_s = (a z_t - b eps) + c2 (x^_k - x^_{k-1}) with x^_k = p z_t - q eps - DPM-Solver++(2M)
               in data-prediction form, second order in the step of lambda = log(alpha / sigma) at no extra network call.

  solver="sde2m"  stochastic multistep rows {a, b, c, c2, p, q} (`multistep_sde_coefficients`): the eta = 1 linear row plus the same
               kind of correction, z_s = ((a z_t - b eps) + c noise) + c2 (x^_k - x^_{k-1}) with c2 = alpha_s (-expm1(-2 h_k)) / (2 r_k)
               - SDE-DPM-Solver++(2M): second order AND noise on the path (what steering needs), at no extra network call.

Which K, eta and solver keep sample quality is a property of the trained checkpoint: nothing here can tell.
"""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Optional, Sequence

import numpy as np
import torch
import torch.nn.functional as F

from .noise_model import step_coefficients

SPACINGS = ("uniform", "quadratic")
SOLVERS = (None, "ddim", "dpm2m", "sde2m")


class Multistep(NamedTuple):
    """What travels in the place of `eta` when a second-order multistep solver is asked for (`check_solver`): "dpm2m", or with
    `stochastic` "sde2m"."""
    lower_order_final: bool = True
    stochastic: bool = False


def check_solver(solver, eta=None, lower_order_final=True) -> Optional[Multistep]:
    """None for the first-order code path (solver None or "ddim"), else the `Multistep` of "dpm2m", which takes no noise on the
    path: an explicit eta other than 0 is a ValueError - or of "sde2m", whose noise is the ancestral one: an explicit eta other
    than 1 is a ValueError."""
    if solver not in SOLVERS:
        raise ValueError(f"solver must be one of {SOLVERS}, got {solver!r}")
    if solver == "sde2m":
        if eta is not None and check_eta(eta) != 1.0:
            raise ValueError(f"solver 'sde2m' draws the ancestral noise (eta = 1), got eta = {eta!r}")
        return Multistep(bool(lower_order_final), True)
    if solver != "dpm2m":
        return None
    if eta is not None and check_eta(eta) != 0.0:
        raise ValueError(f"solver 'dpm2m' is deterministic (eta = 0), got eta = {eta!r}")
    return Multistep(bool(lower_order_final))


def _check_T_K(T, K) -> "tuple[int, int]":
    if isinstance(K, bool) or not isinstance(K, (int, np.integer)):
        raise ValueError(f"steps must be an integer, got {K!r}")
    T, K = int(T), int(K)
    if T < 1:
        raise ValueError(f"timesteps must be >= 1, got {T}")
    if K < 1 or K > T:
        raise ValueError(f"steps must be in 1 .. {T} (the trained grid), got {K}")
    return T, K


def uniform_path(T: int, K: int) -> List[int]:
    """t_k = T - round_half_up(k T / K) in integer arithmetic: strictly monotone for every 1 <= K <= T (consecutive values of
    k T / K differ by T / K >= 1), the identity path for K = T."""
    T, K = _check_T_K(T, K)
    return [T - (2 * k * T + K) // (2 * K) for k in range(K + 1)]


def quadratic_path(T: int, K: int) -> List[int]:
    """t_k ~ T ((K - k) / K)^2: denser near t = 0 (the usual DDIM alternative).  Built from the t = 0 end upwards with
    t_k = min(max(round(.), t_{k+1} + 1), T - k), which is strictly monotone and ends in T by construction."""
    T, K = _check_T_K(T, K)
    path = [0] * (K + 1)
    for k in range(K - 1, -1, -1):
        j = K - k
        raw = (2 * T * j * j + K * K) // (2 * K * K)              # round_half_up(T j^2 / K^2)
        path[k] = min(max(raw, path[k + 1] + 1), T - k)
    return path


def explicit_path(T: int, timesteps: Sequence[int]) -> List[int]:
    """A caller's own list, validated: integers, first T, last 0, strictly decreasing."""
    T = int(T)
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
        out.append(int(v))
    if len(out) < 2 or out[0] != T or out[-1] != 0:
        raise ValueError(f"timesteps must start at {T} and end at 0, got {out[:1]} .. {out[-1:]}")
    if any(b >= a for a, b in zip(out[:-1], out[1:])):
        raise ValueError("timesteps must be strictly decreasing")
    return out


def build_path(T: int, steps: Optional[int] = None, spacing: str = "uniform", timesteps: Optional[Sequence[int]] = None) -> List[int]:
    """The path for `steps` transitions with the given spacing, or the validated explicit `timesteps`."""
    if steps is not None and timesteps is not None:
        raise ValueError("give either steps or timesteps, not both")
    if timesteps is not None:
        return explicit_path(T, timesteps)
    if steps is None:
        steps = int(T)
    if spacing == "uniform":
        return uniform_path(T, steps)
    if spacing == "quadratic":
        return quadratic_path(T, steps)
    raise ValueError(f"spacing must be one of {SPACINGS}, got {spacing!r}")


def check_eta(eta) -> float:
    try:
        e = float(eta)
    except (TypeError, ValueError):
        raise ValueError(f"eta must be a number in [0, 1], got {eta!r}") from None
    if not (0.0 <= e <= 1.0):
        raise ValueError(f"eta must be in [0, 1], got {eta!r}")
    return e


def linear_coefficients(gamma_s: torch.Tensor, gamma_t: torch.Tensor, eta: float) -> torch.Tensor:
    """[rows, 4] float64 {a, b, c, sigma_s^2 - sigma~^2} of z_s = a z_t - b eps + c noise (module docstring)."""
    gs, gt = gamma_s.reshape(-1).to(torch.float64), gamma_t.reshape(-1).to(torch.float64)
    alpha_s, alpha_t = torch.sqrt(torch.sigmoid(-gs)), torch.sqrt(torch.sigmoid(-gt))
    sigma2_s, sigma_t = torch.sigmoid(gs), torch.sqrt(torch.sigmoid(gt))
    sigma2_ts = -torch.expm1(F.softplus(gs) - F.softplus(gt))
    sig = float(eta) * torch.sqrt(sigma2_ts) * torch.sqrt(sigma2_s) / sigma_t
    rest = sigma2_s - sig * sig
    a = alpha_s / alpha_t
    b = a * sigma_t - torch.sqrt(torch.clamp(rest, min=0.0))
    return torch.stack([a, b, sig, rest], dim=1)


def multistep_coefficients(gamma: torch.Tensor, path: Sequence[int], lower_order_final: bool = True) -> torch.Tensor:
    """[K, 5] float64 rows {a, b, c2, p, q} of the DPM-Solver++(2M) update along a descending `path` through the gamma grid:
        x^_k = p z_t - q eps,   z_s = (a z_t - b eps) + c2 (x^_k - x^_{k-1}),
    a, b the eta = 0 row of `linear_coefficients`, p = 1 / alpha_t, q = sigma_t / alpha_t and, with lambda = -gamma / 2 and
    h_k = lambda_s - lambda_t, r_k = h_{k-1} / h_k, c2 = alpha_s (-expm1(-h_k)) / (2 r_k); c2 = 0 on the first transition (no history)
    and, with `lower_order_final`, on the last.  ValueError unless every h_k > 0 (gamma strictly increasing along the path upwards).
    Round to fp32 once, where the rows are uploaded."""
    idx = torch.as_tensor([int(v) for v in path], dtype=torch.int64)
    if idx.numel() < 2:
        raise ValueError("a path holds at least one transition")
    g = torch.as_tensor(gamma).reshape(-1).to(torch.float64)
    gt, gs = g[idx[:-1]], g[idx[1:]]
    hk = (gt - gs) / 2
    if not bool((hk > 0).all()):
        raise ValueError("solver 'dpm2m' needs a gamma grid that increases strictly along the path (some step of "
                         "lambda = log(alpha / sigma) is <= 0)")
    lin = linear_coefficients(gs, gt, 0.0)
    alpha_s, alpha_t = torch.sqrt(torch.sigmoid(-gs)), torch.sqrt(torch.sigmoid(-gt))
    c2 = torch.zeros_like(hk)
    c2[1:] = alpha_s[1:] * (-torch.expm1(-hk[1:])) / (2 * (hk[:-1] / hk[1:]))
    if lower_order_final:
        c2[-1] = 0.0
    return torch.stack([lin[:, 0], lin[:, 1], c2, 1.0 / alpha_t, torch.sqrt(torch.sigmoid(gt)) / alpha_t], dim=1)


def multistep_sde_coefficients(gamma: torch.Tensor, path: Sequence[int], lower_order_final: bool = True) -> torch.Tensor:
    """[K, 6] float64 rows {a, b, c, c2, p, q} of the SDE-DPM-Solver++(2M) update along a descending `path`:
        x^_k = p z_t - q eps,   z_s = ((a z_t - b eps) + c noise) + c2 (x^_k - x^_{k-1}),
    a, b, c the eta = 1 row of `linear_coefficients` (c = sigma_s sqrt(1 - exp(-2 h_k)) is the ancestral sigma~), p and q as in
    `multistep_coefficients` and c2 = alpha_s (-expm1(-2 h_k)) / (2 r_k): twice the step in the exponent, because the noise
    takes the other half of the contraction.  c2 = 0 on the first transition and, with `lower_order_final`, on the last.
    ValueError unless every h_k > 0.  Round to fp32 once, where the rows are uploaded."""
    idx = torch.as_tensor([int(v) for v in path], dtype=torch.int64)
    if idx.numel() < 2:
        raise ValueError("a path holds at least one transition")
    g = torch.as_tensor(gamma).reshape(-1).to(torch.float64)
    gt, gs = g[idx[:-1]], g[idx[1:]]
    hk = (gt - gs) / 2
    if not bool((hk > 0).all()):
        raise ValueError("solver 'sde2m' needs a gamma grid that increases strictly along the path (some step of "
                         "lambda = log(alpha / sigma) is <= 0)")
    lin = linear_coefficients(gs, gt, 1.0)
    alpha_s, alpha_t = torch.sqrt(torch.sigmoid(-gs)), torch.sqrt(torch.sigmoid(-gt))
    c2 = torch.zeros_like(hk)
    c2[1:] = alpha_s[1:] * (-torch.expm1(-2 * hk[1:])) / (2 * (hk[:-1] / hk[1:]))
    if lower_order_final:
        c2[-1] = 0.0
    return torch.stack([lin[:, 0], lin[:, 1], lin[:, 2], c2, 1.0 / alpha_t, torch.sqrt(torch.sigmoid(gt)) / alpha_t], dim=1)


@torch.no_grad()
def path_tables(gamma: torch.Tensor, path: Sequence[int], eta: Optional[float] = None, solver: Optional[str] = None,
                lower_order_final: bool = True) -> Dict[str, object]:
    """Rows of a path from the gamma grid [T+1] (fp32, `schedule_tables(...)["gamma"]`): t_idx / s_idx int32 [K], coef fp32 [K,4],
    form (0 ancestral rows, 1 linear rows) and, for eta = 1, the inpainting rows {alpha_s, sigma_s, alpha_t|s, sigma_t|s}.
    solver="dpm2m" (`eta` may also be a `Multistep`): form 2, coef fp32 [K,5] = `multistep_coefficients`, whose a and b are the
    fp32 values of the eta = 0 rows.  solver="sde2m" (a `Multistep` with `stochastic`): form 3, coef fp32 [K,6] =
    `multistep_sde_coefficients`, whose a, b and c are the fp32 values of the eta = 1 linear rows.  eta None: 1 (ancestral, also
    with "sde2m"), or 0 with "dpm2m"."""
    ms = eta if isinstance(eta, Multistep) else check_solver(solver, eta, lower_order_final)
    g = torch.as_tensor(gamma, dtype=torch.float32).reshape(-1, 1)
    idx = torch.as_tensor(list(path), dtype=torch.int64)
    t_idx, s_idx = idx[:-1], idx[1:]
    if ms is not None and ms.stochastic:
        coef = multistep_sde_coefficients(g, path, ms.lower_order_final).to(torch.float32).contiguous()
        return {"t_idx": t_idx.to(torch.int32).contiguous(), "s_idx": s_idx.to(torch.int32).contiguous(), "coef": coef, "form": 3,
                "coef_inpaint": None, "K": int(t_idx.numel()), "eta": 1.0, "solver": "sde2m",
                "lower_order_final": ms.lower_order_final}
    if ms is not None:
        coef = multistep_coefficients(g, path, ms.lower_order_final).to(torch.float32).contiguous()
        return {"t_idx": t_idx.to(torch.int32).contiguous(), "s_idx": s_idx.to(torch.int32).contiguous(), "coef": coef, "form": 2,
                "coef_inpaint": None, "K": int(t_idx.numel()), "eta": 0.0, "solver": "dpm2m",
                "lower_order_final": ms.lower_order_final}
    eta = check_eta(1.0 if eta is None else eta)
    if eta == 1.0:
        # evaluated in ascending s like the plain table (torch's vectorised CPU kernels may round an element differently at
        # another position of the array): for the identity path this IS the call `schedule_tables` makes, so the bits agree
        s_up, t_up = s_idx.flip(0), t_idx.flip(0)
        coef_up = step_coefficients(g[s_up], g[t_up])
        gs = g[s_up].reshape(-1)
        inpaint = torch.stack([torch.sqrt(torch.sigmoid(-gs)), torch.sqrt(torch.sigmoid(gs)), coef_up[:, 0], torch.sqrt(coef_up[:, 1])],
                              dim=1).to(torch.float32).flip(0).contiguous()
        coef = coef_up.flip(0).contiguous()
        form = 0
    else:
        lin = linear_coefficients(g[s_idx], g[t_idx], eta)
        coef = torch.cat([lin[:, :3], torch.zeros_like(lin[:, :1])], dim=1).to(torch.float32).contiguous()
        inpaint, form = None, 1
    return {"t_idx": t_idx.to(torch.int32).contiguous(), "s_idx": s_idx.to(torch.int32).contiguous(), "coef": coef, "form": form,
            "coef_inpaint": inpaint, "K": int(t_idx.numel()), "eta": eta}


# ----------------------------------------------------------------------------- editing given molecules: partial and ascending paths
# A partial path starts at a grid index `start` <= T instead of T (the reverse chain below a noised molecule); an ascending path is
# one reversed (the eta = 0 update run upwards in t, "DDIM inversion").  Which start, K and eta are chemically useful is, again, a
# property of the trained checkpoint.

def _check_start(T, start, what: str = "start") -> "tuple[int, int]":
    if isinstance(start, bool) or not isinstance(start, (int, np.integer)):
        raise ValueError(f"{what} must be an integer, got {start!r}")
    T, start = int(T), int(start)
    if T < 1:
        raise ValueError(f"timesteps must be >= 1, got {T}")
    if not (1 <= start <= T):
        raise ValueError(f"{what} must be in 1 .. {T} (the trained grid), got {start}")
    return T, start


def partial_path(T: int, start: int, steps: Optional[int] = None, spacing: str = "uniform",
                 timesteps: Optional[Sequence[int]] = None) -> List[int]:
    """Strictly decreasing from `start` (1 <= start <= T) to 0 in K <= start transitions: the builders' formulas with T replaced by
    `start` (default K = start: every grid point below it), or the validated explicit `timesteps`, which must begin at `start`.
    start = T is `build_path`."""
    T, start = _check_start(T, start)
    if steps is not None and timesteps is not None:
        raise ValueError("give either steps or timesteps, not both")
    return build_path(start, steps, spacing, timesteps)


def ascending_path(T: int, end: int, steps: Optional[int] = None, spacing: str = "uniform",
                   timesteps: Optional[Sequence[int]] = None) -> List[int]:
    """`partial_path(T, end, ...)` reversed: strictly increasing from 0 to `end`.  An explicit `timesteps` is given in the
    descending order of `partial_path`."""
    _check_start(T, end, "end")
    return partial_path(T, end, steps, spacing, timesteps)[::-1]


def inversion_coefficients(gamma_u: torch.Tensor, gamma_v: torch.Tensor) -> torch.Tensor:
    """[rows, 2] float64 {a, b} of the upward noise-free update z_v = a z_u - b eps for u < v: a = alpha_v / alpha_u,
    b = a sigma_u - sigma_v - the eta = 0 row of `linear_coefficients` with the roles of s and t exchanged, so that with the same
    eps the down row (v -> u) undoes it.  Round to fp32 once, where the rows are uploaded."""
    gu, gv = gamma_u.reshape(-1).to(torch.float64), gamma_v.reshape(-1).to(torch.float64)
    a = torch.sqrt(torch.sigmoid(-gv)) / torch.sqrt(torch.sigmoid(-gu))
    b = a * torch.sqrt(torch.sigmoid(gu)) - torch.sqrt(torch.sigmoid(gv))
    return torch.stack([a, b], dim=1)


@torch.no_grad()
def up_tables(gamma: torch.Tensor, path: Sequence[int]) -> Dict[str, object]:
    """Arrays of hd_set_path_up for an ascending `path` (0 = path[0] < .. < path[K] <= T) from the gamma grid [T+1] (fp32):
    from_idx / to_idx int32 [K], coef fp32 [K,4] = {a, b, 0, 0}."""
    idx = [int(v) for v in path]
    if len(idx) < 2 or any(b <= a for a, b in zip(idx[:-1], idx[1:])):
        raise ValueError("an ascending path must be strictly increasing and hold at least one transition")
    g = torch.as_tensor(gamma, dtype=torch.float32).reshape(-1)
    if idx[0] < 0 or idx[-1] >= g.numel():
        raise ValueError(f"an ascending path must stay within 0 .. {g.numel() - 1}")
    idx_t = torch.as_tensor(idx, dtype=torch.int64)
    u, v = idx_t[:-1], idx_t[1:]
    ab = inversion_coefficients(g[u], g[v])
    coef = torch.cat([ab, torch.zeros_like(ab)], dim=1).to(torch.float32).contiguous()
    return {"from_idx": u.to(torch.int32).contiguous(), "to_idx": v.to(torch.int32).contiguous(), "coef": coef, "K": int(u.numel())}


# ----------------------------------------------------------------------------- recording a trajectory (the reference's sample_chain)
# en_diffusion.py:669-710 keeps `keep` frames of a T-step chain: after the step that arrives at s it writes z_s into
# chain[(s * keep) // T], later writes overwriting earlier ones, and frame 0 ends up holding the decoded (x, h).

class ChainFrames(NamedTuple):
    frame_of: List[int]     # [K] frame transition k writes, -1: none
    frame_t: List[int]      # [keep] fine-grid timestep every frame's state has arrived at


def chain_frames(K, keep, path: Optional[Sequence[int]] = None) -> ChainFrames:
    """Which frame each of the K transitions of a path records.  Transition k arrives at path position p = K - 1 - k (counted from
    the t = 0 end, as the reference counts s), whose frame is (p * keep) // K; only the LAST transition of a frame keeps its entry,
    the others get -1 - the reference's last-write-wins with one write per frame.  1 <= keep <= K, so every frame is claimed
    exactly once; on the identity path (K = T, p = s) this is the reference's formula.  `frame_t[f]` is the grid index the claiming
    transition arrives at: `path[k + 1]` of the descending `path` (K + 1 entries; None: the identity path K, K - 1, .., 0)."""
    for name, v in (("steps", K), ("keep_frames", keep)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{name} must be an integer, got {v!r}")
    K, keep = int(K), int(keep)
    if K < 1:
        raise ValueError(f"a path holds at least one transition, got {K}")
    if not (1 <= keep <= K):
        raise ValueError(f"keep_frames must be in 1 .. {K} (the chain's transitions), got {keep}")
    path = list(range(K, -1, -1)) if path is None else [int(v) for v in path]
    if len(path) != K + 1:
        raise ValueError(f"path must hold {K} + 1 grid indices, got {len(path)}")
    last = [-1] * keep
    for k in range(K):                                   # ascending k: the last writer of a frame stays
        last[((K - 1 - k) * keep) // K] = k
    frame_of = [-1] * K
    for f, k in enumerate(last):
        frame_of[k] = f
    return ChainFrames(frame_of, [path[k + 1] for k in last])
