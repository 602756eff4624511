"""Restraint-guided sampling: host side (the tables, argument resolution, the per-transition rows).

At every transition of a path loop an energy U is evaluated on the network's data prediction x^0 and its gradient goes into the noise
prediction (hd_restraint_attach / hd_set_restraint / k_restrain_eps, include/hierdiff_hip.h); the update that follows is unchanged.

    U_obs  = 1/2 sum_{i valid} sum_p k_p max(0, r_p - |x_i - y_p|)^2                  stay out of these spheres
    U_pair = 1/2 sum_q k_q (max(0, d - hi)^2 + max(0, lo - d)^2),  d = |x_i - x_j|     keep two nodes lo .. hi apart
    U_anc  = 1/2 sum_a k_a max(0, |x_i - a| - r)^2                                     put a node within r of a point

THE FRAME.  Coordinates are x = norm_values[0] * z_x.  There are two frames the tables can be read in (`restraint_frame`):

  "model" (the default, everywhere)   the MODEL'S frame, which has the centre of mass of the molecule's valid nodes at the origin -
      during the whole chain and in the result.  Obstacles and anchors are given in that frame: place the pocket relative to where
      the ligand's centre should sit.  Nothing translates them.
  "known" (sample_inpaint / sample_grow / inpaint_steps only)   the frame of the call's `x_known`, as given - the coordinates the
      scaffold was cut out in, a pocket's for instance.  Inpainting returns the known fragments as a pure translation of the input,
      so it is the one mode with an absolute frame.  At every transition, with F the molecule's valid fixed nodes,
          tau = mean_F(x^0) - mean_F(x_known)         the position of node i in the user's coordinates is x^0_i - tau
      and the obstacle and anchor terms are evaluated on x^0_i - (y + tau) (pairs do not see tau).  The gradient is taken with tau
      held constant and for FREE nodes only: a fixed node's step is 0 by definition - the block is the frame, and its own clashes
      are the user's input; a pair between a free and a fixed node acts on the free one.  The mean of the clipped steps over ALL valid
      nodes is then removed from every valid node (fixed nodes receive -mean), so eps^_x stays mean-free as the chain requires; behind
      the posterior step and the replacement - which puts the block where the generated fixed rows' centre went - a free node has
      moved relative to the block by exactly its own step times the update's coefficient.  A molecule without fixed nodes has
      tau = 0: today's update.  Results carry 'frame_shift' (tau of the returned x) and 'x_known_frame' = x - tau, the molecule in
      the coordinates of the input.

FIELDS.  `Field` is a scalar potential on a regular 3-D lattice - an AutoDock-style affinity map, or any field the user rasterises
(`Field.from_obstacles` turns the sphere energy above into one) - read by trilinear interpolation: 8 loads per node whatever the
potential was made from, any shape, negative (attractive) values included.  For a valid node at x, with p = x - tau (tau = 0 in the
model's frame, the tau above in the known frame), origin o, spacing h, lattice v [n0, n1, n2], per axis c in double:

    u_c = (p_c - o_c) / h_c,  ub_c = min(max(u_c, 0), n_c - 1),  cell_c = min(floor(ub_c), n_c - 2),  t_c = ub_c - cell_c
    V   = sum_{a,b,c in {0,1}} v[cell_0 + a, cell_1 + b, cell_2 + c] W_a(t_0) W_b(t_1) W_c(t_2),   W_0(t) = 1 - t, W_1(t) = t
    out_c = (u_c - ub_c) h_c                                  how far outside the box, data units; 0 inside
    E   = k w_i (V + 1/2 wall sum_c out_c^2),    U_fld = sum over the fields and the valid nodes

    dE/dx_c = k w_i ([0 <= u_c <= n_c - 1] dV/dt_c / h_c + wall out_c): on an interior lattice plane the gradient is the right-hand
cell's, at u_c = n_c - 1 the last cell's with t = 1; outside the box an axis contributes only the wall.  A node with a non-finite
coordinate contributes neither energy nor gradient.  U_fld may be negative.  In every other respect the term follows the obstacles:
the gradient joins the same per-node step ahead of the clip and the mean; in the known frame only free nodes gather it and the
energy sums over all valid nodes.  Values are shared by the molecules of a call, weights may differ per molecule; a call carries at
most MAX_FIELDS fields.

TEMPLATES.  `Template` asks for a 3-D arrangement of named nodes "wherever and however the molecule ends up oriented": at every
transition the data prediction is superposed rigidly (Kabsch) on the template and the residual of the best fit is the restraint.  Rows
(i_m, y_m, w_m); a row is active when node i_m exists and is valid in the molecule and w_m > 0.  Over the active rows, in double:

    W = sum w_m,  c_x = sum w_m x_{i_m} / W,  c_y = sum w_m y_m / W,  x'_m = x_{i_m} - c_x,  y'_m = y_m - c_y
    S = sum w_m x'_m y'_m^T,  R = argmax_{R in SO(3)} tr(R^T S)   ("translation": R = I)
    r_m = x'_m - R y'_m,  U_tpl = 1/2 k sum w_m |r_m|^2,  rmsd = sqrt(sum w_m |r_m|^2 / W),  dU_tpl/dx_{i_m} += k w_m r_m

R is a proper rotation, so - unlike O(M^2) pair rows, which see distances only - a mirror image of the template does not fit.  The
gradient is exact: R maximises, so its dependence on x drops out.  No weight, exactly one active row or a non-finite active coordinate:
the template contributes nothing to that molecule.  With two active rows or collinear ones R is not unique; the energy still is.  A
template carries its own frame and never sees tau; in the known frame rows on fixed nodes take part in the fit, only free nodes gather
a gradient.  The fit's by-product is an absolute frame: results carry 'x_template_frame' = R^T (x - c_x) + c_y of the first template -
the molecule in the template's coordinates, a pocket's if that is where the template came from.  A call carries at most MAX_TEMPLATES.
Out of scope: obstacles or fields read in the fitted frame (their gradient would need dR/dx), flat-bottomed templates, scaling fits,
correspondence search (rows name their nodes), templates on h.

FEATURES.  `Features` restrains the other F columns of a coarse molecule - the property and embedding channels h that the stage-2
decoder reads - softly, where `fixed_h_mask` can only replace.  With v_ic the data prediction of channel c of the valid node i in data
units (the value a record="x0" frame shows: v = (1 / alpha_t (z - sigma_t eps^)) nv1 + nb1, nv1 = norm_values[1], nb1 =
norm_biases[1]), in double:

    bands   lo, hi, k [W, F] (nodes i >= W have none); element (i, c) is active when k_ic > 0 and v_ic is finite
            U_band = 1/2 sum k_ic (max(0, v - hi)^2 + max(0, lo - v)^2)      lo = -inf / hi = inf: one-sided; lo = hi: a harmonic target
    sums    at most MAX_FEATURE_SUMS rows `FeatureSum(coef [F], lo, hi, k, reduce)`:  s_r = sum_{i valid} sum_c coef_rc v_ic,
            m_r = s_r ("sum") or s_r / n ("mean", n the valid nodes),  U_sum = 1/2 sum_r k_r (max(0, m_r - hi_r)^2 + max(0, lo_r - m_r)^2)
            a row with k_r = 0, or in a molecule without valid nodes, is inactive; a row that reads a non-finite v contributes nothing

U_feat = U_band + U_sum, and eps^[i, 3 + c] += clip_i(s_b lambda_k ratio dU_feat/dv_ic): s_b and lambda_k as for the positions, ratio =
nv1 / nv0 under the "score" schedule (dv/dz_h = nv1 / alpha_t) and 1 otherwise, the clip on the norm of the node's F steps (apart from
the position step's clip), no mean removed.  Features have no frame: with restraint_frame="known" the term acts on every valid node and
the replacement step overwrites the known elements afterwards.  Steering weighs on the total with U_feat - selection is the safe way
to impose a window on channels that are rounded downstream.  Results carry 'restraint_feature_energy' [2] = (U_band, U_sum) and
'feature_sums' [S] = m_r of the returned h.  Out of scope: per-feature scale or clip keywords (the per-element k does that), node
weights inside sums, products or other nonlinear collective variables, the context column, pocket models, restraints that read the
rounded integer channels.

A pair or anchor row whose node index is -1 (padding), >= the molecule's size or masked is inactive - documented behaviour, not an
error, because `sample` draws the sizes.  A term at distance exactly 0 contributes no gradient.

Everything in this module is host arithmetic except `Restraints.energy` on a device tensor.  Mechanism only: which scale, schedule
and clip steer a trained checkpoint usefully is for the user to validate; synthetic weights say nothing chemical."""
from __future__ import annotations

import math
from typing import Optional, Sequence

import numpy as np
import torch

SCHEDULES = ("score", "sigma")
FRAMES = ("model", "known")
MAX_FIELDS = 8                                   # HD_MAX_FIELDS
MAX_TEMPLATES = 4                                # HD_MAX_TEMPLATES
FITS = ("rigid", "translation")
MAX_FEATURE_SUMS = 8                             # HD_MAX_FEATURE_SUMS
REDUCES = ("sum", "mean")


def check_frame(model, frame) -> int:
    """`restraint_frame` (None: the model's attribute; None there: "model") -> the library's code, 0 "model" or 1 "known"."""
    frame = getattr(model, "restraint_frame", None) if frame is None else frame
    if frame is None:
        return 0
    if not isinstance(frame, str) or frame not in FRAMES:
        raise ValueError(f"restraint_frame must be one of {FRAMES} (or None: the model's), got {frame!r}")
    return FRAMES.index(frame)


def frame_shift(x: torch.Tensor, node_mask: torch.Tensor, fixed_mask: torch.Tensor, x_known: torch.Tensor) -> torch.Tensor:
    """[B, 3] float64 tau = mean_F(x) - mean_F(x_known) over the valid fixed nodes F of every molecule (0 where there is none)."""
    B, N = int(x.shape[0]), int(x.shape[1])
    f = (fixed_mask.reshape(B, N).bool() & node_mask.reshape(B, N).bool()).to(x.device).to(torch.float64).unsqueeze(-1)
    nf = f.sum(1)
    tau = ((x.detach().double() * f).sum(1) - (x_known.detach().to(x.device).double() * f).sum(1)) / nf.clamp(min=1.0)
    return torch.where(nf > 0, tau, torch.zeros_like(tau))


def _table(v, width: int, name: str) -> Optional[torch.Tensor]:
    """None, [n, width] (shared) or [B, n, width] (per molecule) -> a contiguous CPU tensor [rows, n, width]."""
    if v is None:
        return None
    try:
        t = torch.as_tensor(v).detach().cpu()
    except (TypeError, ValueError, RuntimeError):
        raise ValueError(f"{name} must be a tensor or nested list [n, {width}] or [B, n, {width}]") from None
    if t.numel() == 0:
        return None
    if t.dim() == 2:
        t = t.unsqueeze(0)
    if t.dim() != 3 or t.shape[2] != width:
        raise ValueError(f"{name} must be [n, {width}] (shared) or [B, n, {width}] (per molecule), got {tuple(t.shape)}")
    if t.is_floating_point() and not bool(torch.isfinite(t).all()):
        raise ValueError(f"{name} must be finite")
    return t.to(torch.float64)


def _number(v, name: str, positive: bool = False) -> float:
    """A finite number >= 0 (> 0 with `positive`), rounded to fp32 - what the library reads."""
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise ValueError(f"{name} must be a number, got {v!r}")
    f = float(np.float32(v))
    if not math.isfinite(f) or f < 0 or (positive and not f > 0):
        raise ValueError(f"{name} must be finite and {'> 0' if positive else '>= 0'}, got {v!r}")
    return f


class Field:
    """One scalar potential on a regular lattice (module docstring: FIELDS).

    values   [n0, n1, n2] array or tensor, stored as float32; every n_c >= 2, finite, fewer than 2^31 entries
    origin   3 numbers: the position of values[0, 0, 0], data units
    spacing  a number or 3 numbers > 0 (the lattice may be anisotropic)
    k        stiffness >= 0 (the factor in front of the interpolated value), wall: stiffness >= 0 of the harmonic wall outside the box
    weights  None: every valid node weighs 1; [W] (shared) or [B, W] (per molecule), >= 0: node i takes weights[i], nodes i >= W take 0
             (documented behaviour, like an anchor on a node the molecule does not have: `sample` draws the sizes)
    ValueError for every malformed argument, before a device is looked at.  origin, spacing, k and wall are rounded to fp32 once,
    here.  A device copy of the values is kept per device, so a large lattice is uploaded once."""

    def __init__(self, values, origin, spacing, k=1.0, wall=0.0, weights=None):
        try:
            v = torch.as_tensor(np.asarray(values.detach().cpu()) if isinstance(values, torch.Tensor) else np.asarray(values))
        except (TypeError, ValueError, RuntimeError):
            raise ValueError("Field: values must be a 3-D array [n0, n1, n2]") from None
        if v.dim() != 3 or v.dtype == torch.bool or v.is_complex():
            raise ValueError(f"Field: values must be a real 3-D array [n0, n1, n2], got shape {tuple(v.shape)}")
        if min(v.shape) < 2:
            raise ValueError(f"Field: every lattice dimension must be >= 2, got {tuple(v.shape)}")
        if v.numel() >= 2 ** 31:
            raise ValueError("Field: a lattice holds fewer than 2^31 values")
        v = v.to(torch.float32).contiguous()
        if not bool(torch.isfinite(v).all()):
            raise ValueError("Field: values must be finite (in float32)")
        self.values = v
        self.origin = self._three(origin, "origin", False)
        self.spacing = self._three(spacing, "spacing", True)
        self.k, self.wall = _number(k, "Field: k"), _number(wall, "Field: wall")
        self.weights = None
        if weights is not None:
            try:
                w = torch.as_tensor(weights).detach().cpu().to(torch.float32)
            except (TypeError, ValueError, RuntimeError):
                raise ValueError("Field: weights must be None, [W] or [B, W]") from None
            if w.dim() not in (1, 2) or w.numel() == 0:
                raise ValueError(f"Field: weights must be None, [W] or [B, W], got {tuple(w.shape)}")
            if not bool(torch.isfinite(w).all()) or bool((w < 0).any()):
                raise ValueError("Field: weights must be finite and >= 0")
            self.weights = (w.unsqueeze(0) if w.dim() == 1 else w).contiguous()
        self._dev = {}

    @staticmethod
    def _three(v, name: str, scalar_ok: bool) -> torch.Tensor:
        try:
            t = torch.as_tensor(v, dtype=torch.float64).detach().cpu().reshape(-1)
        except (TypeError, ValueError, RuntimeError):
            raise ValueError(f"Field: {name} must be {'a number or ' if scalar_ok else ''}3 numbers, got {v!r}") from None
        if scalar_ok and t.numel() == 1 and torch.as_tensor(v).dim() == 0:
            t = t.repeat(3)
        if t.numel() != 3 or isinstance(v, bool):
            raise ValueError(f"Field: {name} must be {'a number or ' if scalar_ok else ''}3 numbers, got {v!r}")
        t = t.to(torch.float32)
        if not bool(torch.isfinite(t).all()) or (scalar_ok and not bool((t > 0).all())):
            raise ValueError(f"Field: {name} must be finite{' and > 0' if scalar_ok else ''}, got {v!r}")
        return t

    @property
    def rows(self) -> int:
        return 1 if self.weights is None else int(self.weights.shape[0])

    def geom(self) -> torch.Tensor:
        """[8] float32 (o, h, k, wall): the library's row."""
        return torch.cat([self.origin, self.spacing, torch.tensor([self.k, self.wall], dtype=torch.float32)])

    def node_weights(self, N: int) -> torch.Tensor:
        """[rows, N] float32: the weights cut or zero-padded to N nodes (None: ones)."""
        if self.weights is None:
            return torch.ones(1, N, dtype=torch.float32)
        w = torch.zeros(self.weights.shape[0], N, dtype=torch.float32)
        n = min(N, int(self.weights.shape[1]))
        w[:, :n] = self.weights[:, :n]
        return w

    def device_values(self, dev) -> torch.Tensor:
        dev = torch.device(dev)
        hit = self._dev.get(dev)
        if hit is None:
            hit = self._dev[dev] = self.values.to(dev).contiguous()
        return hit

    def _slice(self, lo: int, hi: int) -> "Field":
        if self.weights is None or self.weights.shape[0] == 1:
            return self
        out = object.__new__(Field)
        out.__dict__.update(self.__dict__)               # the values and their device copies are shared
        out.weights = self.weights[lo:hi].contiguous()
        return out

    @classmethod
    def from_obstacles(cls, obstacles, origin, shape, spacing, k=1.0, wall=0.0) -> "Field":
        """The sphere energy 1/2 sum_p k_p max(0, r_p - |y - y_p|)^2 of `obstacles` ([P, 5] rows (y, r, k), shared) rasterised at the
        lattice points y = origin + index * spacing of a lattice of `shape` = (n0, n1, n2): float64 on the CPU in chunks, rounded to
        fp32 once.  Between the lattice points the field is the trilinear interpolant, not the sphere energy."""
        obs = _table(obstacles, 5, "obstacles")
        if obs is None or obs.shape[0] != 1:
            raise ValueError("Field.from_obstacles: obstacles must be a non-empty shared table [P, 5]")
        if bool((obs[..., 3:] < 0).any()):
            raise ValueError("obstacles: r and k must be >= 0 (a row with r = 0 or k = 0 is padding)")
        try:
            shape = tuple(int(n) for n in shape)
        except (TypeError, ValueError):
            raise ValueError(f"Field.from_obstacles: shape must be 3 integers >= 2, got {shape!r}") from None
        if len(shape) != 3 or min(shape) < 2 or shape[0] * shape[1] * shape[2] >= 2 ** 31:
            raise ValueError(f"Field.from_obstacles: shape must be 3 integers >= 2 (fewer than 2^31 points), got {shape!r}")
        o = cls._three(origin, "origin", False).double()
        h = cls._three(spacing, "spacing", True).double()
        ob = obs[0].to(torch.float32).double()           # the fp32 rows `Restraints` keeps
        ob = ob[(ob[:, 3] > 0) & (ob[:, 4] > 0)]
        ax = [o[c] + torch.arange(shape[c], dtype=torch.float64) * h[c] for c in range(3)]
        pts = torch.stack(torch.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)
        vals = torch.zeros(pts.shape[0], dtype=torch.float64)
        chunk = max(1, (1 << 22) // max(1, int(ob.shape[0])))
        for lo in range(0, pts.shape[0], chunk):
            d = _norm(pts[lo:lo + chunk, None, :] - ob[None, :, :3])
            vals[lo:lo + chunk] = 0.5 * (ob[None, :, 4] * torch.clamp(ob[None, :, 3] - d, min=0) ** 2).sum(1)
        return cls(vals.reshape(shape).to(torch.float32), origin, spacing, k, wall)


def _fields(fields) -> list:
    if fields is None:
        return []
    fl = [fields] if isinstance(fields, Field) else fields
    if not isinstance(fl, (list, tuple)) or not all(isinstance(f, Field) for f in fl):
        raise ValueError("fields must be a restraints.Field or a list of them")
    if len(fl) > MAX_FIELDS:
        raise ValueError(f"fields: a call carries at most {MAX_FIELDS} fields, got {len(fl)}")
    rows = {f.rows for f in fl} - {1}
    if len(rows) > 1:
        raise ValueError(f"fields: per-molecule weights hold rows for {sorted(rows)} molecules; they must agree")
    return list(fl)


class Template:
    """One rigid template (module docstring: TEMPLATES).

    index      [M] (shared) or [B, M] (per molecule) node indices, integers >= 0, or -1 for padding
    positions  [M, 3] or [B, M, 3] template positions y_m, data units, finite (rounded to fp32 once, here)
    weights    None: every row weighs 1; [M] or [B, M], finite and >= 0 (a row with w = 0 is inactive)
    k          stiffness >= 0 (k = 0: no force, but the fit and 'x_template_frame' are still reported)
    fit        "rigid" (rotation and translation) or "translation" (R = I)
    If any of the three arrays has the batch axis, the others are repeated for every molecule.  ValueError for every malformed
    argument, before a device is looked at."""

    def __init__(self, index, positions, weights=None, k=1.0, fit="rigid"):
        def arr(v, name, dtype=torch.float64):
            if isinstance(v, bool):
                raise ValueError(f"Template: {name} must be an array, got {v!r}")
            try:
                return torch.as_tensor(v).detach().cpu().to(dtype)
            except (TypeError, ValueError, RuntimeError):
                raise ValueError(f"Template: {name} must be a tensor or nested list of numbers") from None
        idx, pos = arr(index, "index"), arr(positions, "positions")
        if idx.dim() not in (1, 2) or idx.numel() == 0:
            raise ValueError(f"Template: index must be [M] (shared) or [B, M] (per molecule) with M >= 1, got {tuple(idx.shape)}")
        if not bool(torch.isfinite(idx).all()) or bool((idx != idx.round()).any()) or bool((idx < -1).any()):
            raise ValueError("Template: node indices must be integers >= 0, or -1 for padding")
        M = int(idx.shape[-1])
        if pos.dim() not in (2, 3) or tuple(pos.shape[-2:]) != (M, 3):
            raise ValueError(f"Template: positions must be [{M}, 3] (shared) or [B, {M}, 3] (per molecule), got {tuple(pos.shape)}")
        pos = pos.to(torch.float32)
        if not bool(torch.isfinite(pos).all()):
            raise ValueError("Template: positions must be finite (in float32)")
        if weights is None:
            w = torch.ones(M, dtype=torch.float32)
        else:
            w = arr(weights, "weights").to(torch.float32)
            if w.dim() not in (1, 2) or int(w.shape[-1]) != M:
                raise ValueError(f"Template: weights must be None, [{M}] or [B, {M}], got {tuple(w.shape)}")
            if not bool(torch.isfinite(w).all()) or bool((w < 0).any()):
                raise ValueError("Template: weights must be finite and >= 0")
        idx = idx.unsqueeze(0) if idx.dim() == 1 else idx
        pos = pos.unsqueeze(0) if pos.dim() == 2 else pos
        w = w.unsqueeze(0) if w.dim() == 1 else w
        rows = {int(t.shape[0]) for t in (idx, pos, w)} - {1}
        if len(rows) > 1:
            raise ValueError(f"Template: index, positions and weights hold rows for {sorted(rows)} molecules; they must agree")
        r = max(rows | {1})
        self.index = idx.to(torch.int32).expand(r, M).contiguous()
        self.positions = pos.expand(r, M, 3).contiguous()
        self.weights = w.expand(r, M).contiguous()
        self.k = _number(k, "Template: k")
        if not isinstance(fit, str) or fit not in FITS:
            raise ValueError(f"Template: fit must be one of {FITS}, got {fit!r}")
        self.fit = fit

    @property
    def rows(self) -> int:
        return int(self.index.shape[0])

    @property
    def M(self) -> int:
        return int(self.index.shape[1])

    def _slice(self, lo: int, hi: int) -> "Template":
        if self.rows == 1:
            return self
        out = object.__new__(Template)
        out.__dict__.update(self.__dict__)
        out.index, out.positions, out.weights = (t[lo:hi].contiguous() for t in (self.index, self.positions, self.weights))
        return out


def _templates(templates) -> list:
    if templates is None:
        return []
    tl = [templates] if isinstance(templates, Template) else templates
    if not isinstance(tl, (list, tuple)) or not all(isinstance(t, Template) for t in tl):
        raise ValueError("templates must be a restraints.Template or a list of them")
    if len(tl) > MAX_TEMPLATES:
        raise ValueError(f"templates: a call carries at most {MAX_TEMPLATES} templates, got {len(tl)}")
    rows = {t.rows for t in tl} - {1}
    if len(rows) > 1:
        raise ValueError(f"templates: per-molecule rows are given for {sorted(rows)} molecules; they must agree")
    return list(tl)


def _no_none(v, fill: float):
    """Nested lists with None (JSON's null: no bound) -> the same with `fill`."""
    if isinstance(v, (list, tuple)):
        return [_no_none(e, fill) for e in v]
    return fill if v is None else v


def _bound(v, fill: float, name: str) -> torch.Tensor:
    """A bound (None: `fill`, -inf or inf; inside nested lists too) as a float32 CPU tensor; +-inf are allowed, NaN is not."""
    if v is None:
        return torch.tensor(fill, dtype=torch.float32)
    v = _no_none(v, fill)
    if isinstance(v, bool):
        raise ValueError(f"{name} must be a number or an array, got {v!r}")
    try:
        t = torch.as_tensor(np.array(v) if isinstance(v, np.ndarray) else v).detach().cpu().to(torch.float64).to(torch.float32)
    except (TypeError, ValueError, RuntimeError):
        raise ValueError(f"{name} must be a number or an array of numbers") from None
    if bool(torch.isnan(t).any()):
        raise ValueError(f"{name} must not be NaN (None or +-inf: no bound)")
    return t


class FeatureSum:
    """One molecule-wide sum restraint (module docstring: FEATURES).

    coef    [F] finite coefficients of the feature channels
    lo, hi  a number (shared) or [B] (per molecule); None: -inf / +inf
    k       stiffness >= 0, finite (0: the row is inactive, its m_r is still not reported)
    reduce  "sum" or "mean" (s_r / the molecule's valid nodes)
    ValueError for every malformed argument, before a device is looked at.  Everything is rounded to fp32 once, here."""

    def __init__(self, coef, lo=None, hi=None, k=1.0, reduce="sum"):
        if isinstance(coef, bool):
            raise ValueError(f"FeatureSum: coef must be [F] numbers, got {coef!r}")
        try:
            c = torch.as_tensor(coef).detach().cpu().to(torch.float64).to(torch.float32)
        except (TypeError, ValueError, RuntimeError):
            raise ValueError("FeatureSum: coef must be [F] numbers") from None
        if c.dim() != 1 or c.numel() == 0:
            raise ValueError(f"FeatureSum: coef must be [F], got {tuple(c.shape)}")
        if not bool(torch.isfinite(c).all()):
            raise ValueError("FeatureSum: coef must be finite")
        self.coef = c.contiguous()
        lo_, hi_ = _bound(lo, -math.inf, "FeatureSum: lo"), _bound(hi, math.inf, "FeatureSum: hi")
        if lo_.dim() > 1 or hi_.dim() > 1:
            raise ValueError("FeatureSum: lo and hi must be a number or [B]")
        rows = {int(t.numel()) for t in (lo_, hi_) if t.dim() == 1} - {1}
        if len(rows) > 1:
            raise ValueError(f"FeatureSum: lo and hi hold rows for {sorted(rows)} molecules; they must agree")
        r = max(rows | {1})
        self.lo, self.hi = lo_.reshape(-1).expand(r).contiguous(), hi_.reshape(-1).expand(r).contiguous()
        if bool((self.lo > self.hi).any()):
            raise ValueError("FeatureSum: lo > hi")
        self.k = _number(k, "FeatureSum: k")
        if not isinstance(reduce, str) or reduce not in REDUCES:
            raise ValueError(f"FeatureSum: reduce must be one of {REDUCES}, got {reduce!r}")
        self.reduce = reduce

    @property
    def rows(self) -> int:
        return int(self.lo.shape[0])

    @property
    def F(self) -> int:
        return int(self.coef.shape[0])

    def _slice(self, lo: int, hi: int) -> "FeatureSum":
        if self.rows == 1:
            return self
        out = object.__new__(FeatureSum)
        out.__dict__.update(self.__dict__)
        out.lo, out.hi = self.lo[lo:hi].contiguous(), self.hi[lo:hi].contiguous()
        return out


class Features:
    """Bands and sums on the features h (module docstring: FEATURES).

    lo, hi  [W, F] (shared) or [B, W, F] (per molecule); None: -inf / +inf (both None: no bands)
    k       stiffness >= 0, finite: a number or anything that broadcasts to the bands' shape (k_ic = 0: the element is inactive)
    sums    a `FeatureSum` or a sequence of at most MAX_FEATURE_SUMS of them
    ValueError for every malformed argument, before a device is looked at.  Everything is rounded to fp32 once, here."""

    def __init__(self, lo=None, hi=None, k=1.0, sums=()):
        sl = [sums] if isinstance(sums, FeatureSum) else sums
        if sl is None:
            sl = []
        if not isinstance(sl, (list, tuple)) or not all(isinstance(r, FeatureSum) for r in sl):
            raise ValueError("Features: sums must be a restraints.FeatureSum or a sequence of them")
        if len(sl) > MAX_FEATURE_SUMS:
            raise ValueError(f"Features: a call carries at most {MAX_FEATURE_SUMS} sums, got {len(sl)}")
        self.sums = list(sl)
        self.lo = self.hi = self.k = None
        if lo is not None or hi is not None:
            lo_, hi_ = _bound(lo, -math.inf, "Features: lo"), _bound(hi, math.inf, "Features: hi")
            shape = lo_.shape if lo is not None else hi_.shape
            if len(shape) not in (2, 3) or 0 in shape or (lo is not None and hi is not None and lo_.shape != hi_.shape):
                raise ValueError(f"Features: lo and hi must be [W, F] (shared) or [B, W, F] (per molecule) and agree, got "
                                 f"{tuple(lo_.shape) if lo is not None else None} and {tuple(hi_.shape) if hi is not None else None}")
            if isinstance(k, bool):
                raise ValueError(f"Features: k must be a number or an array, got {k!r}")
            try:
                k_ = torch.as_tensor(k).detach().cpu().to(torch.float64).to(torch.float32)
                k_ = k_.expand(shape)
            except (TypeError, ValueError, RuntimeError):
                raise ValueError(f"Features: k must be a number or broadcast to the bands' shape {tuple(shape)}") from None
            if not bool(torch.isfinite(k_).all()) or bool((k_ < 0).any()):
                raise ValueError("Features: k must be finite and >= 0")
            lo_, hi_ = lo_.expand(shape), hi_.expand(shape)
            if bool((lo_ > hi_).any()):
                raise ValueError("Features: lo > hi")
            three = (lambda t: (t.unsqueeze(0) if t.dim() == 2 else t).contiguous())
            self.lo, self.hi, self.k = three(lo_), three(hi_), three(k_)
        elif not self.sums:
            raise ValueError("Features: give bands (lo / hi) or sums")
        fs = {r.F for r in self.sums} | ({int(self.lo.shape[2])} if self.lo is not None else set())
        if len(fs) > 1:
            raise ValueError(f"Features: the bands and the sums name {sorted(fs)} feature channels; they must agree")
        rows = {r.rows for r in self.sums} - {1}
        if len(rows) > 1:
            raise ValueError(f"Features: per-molecule sum bounds are given for {sorted(rows)} molecules; they must agree")

    @classmethod
    def target(cls, values, k=1.0, tol=0.0, sums=()) -> "Features":
        """Harmonic targets: lo = values - tol, hi = values + tol (tol >= 0: a number or anything that broadcasts)."""
        v = _bound(values, 0.0, "Features.target: values")
        if values is None or not bool(torch.isfinite(v).all()):
            raise ValueError("Features.target: values must be finite [W, F] or [B, W, F]")
        t = _bound(tol, 0.0, "Features.target: tol")
        if tol is None or not bool(torch.isfinite(t).all()) or bool((t < 0).any()):
            raise ValueError("Features.target: tol must be finite and >= 0")
        try:
            t = t.expand(v.shape)
        except RuntimeError:
            raise ValueError("Features.target: tol must broadcast to the values' shape") from None
        return cls(v - t, v + t, k, sums)

    @property
    def F(self) -> int:
        return int(self.lo.shape[2]) if self.lo is not None else self.sums[0].F

    @property
    def W(self) -> int:
        return 0 if self.lo is None else int(self.lo.shape[1])

    @property
    def S(self) -> int:
        return len(self.sums)

    def band_rows(self) -> int:
        return 1 if self.lo is None else int(self.lo.shape[0])

    def sum_rows(self) -> int:
        return max([r.rows for r in self.sums] + [1])

    def tables(self):
        """(lo, hi, k [band_rows, W, F], coef [sum_rows, S, F], sum_f [sum_rows, S, 4] = (lo, hi, k, reduce)) float32: the library's."""
        F, S, sr = self.F, self.S, self.sum_rows()
        if self.lo is None:
            lo = hi = k = torch.zeros((1, 0, F), dtype=torch.float32)
        else:
            lo, hi, k = self.lo, self.hi, self.k
        coef = torch.zeros((sr, S, F), dtype=torch.float32)
        f = torch.zeros((sr, S, 4), dtype=torch.float32)
        for j, r in enumerate(self.sums):
            coef[:, j] = r.coef
            f[:, j, 0], f[:, j, 1], f[:, j, 2], f[:, j, 3] = r.lo, r.hi, r.k, float(REDUCES.index(r.reduce))
        return lo.contiguous(), hi.contiguous(), k.contiguous(), coef.contiguous(), f.contiguous()

    def _slice(self, lo: int, hi: int) -> "Features":
        out = object.__new__(Features)
        out.__dict__.update(self.__dict__)
        if self.lo is not None and self.lo.shape[0] != 1:
            out.lo, out.hi, out.k = (t[lo:hi].contiguous() for t in (self.lo, self.hi, self.k))
        out.sums = [r._slice(lo, hi) for r in self.sums]
        return out

    @classmethod
    def from_dict(cls, d, where: str = "features") -> "Features":
        """{"bands": {"lo", "hi", "k"} | {"target", "tol", "k"}, "sums": [{"coef", "lo", "hi", "k", "reduce"}]} (each part optional)."""
        if not isinstance(d, dict) or set(d) - {"bands", "sums"}:
            raise ValueError(f"{where}: features is an object with the keys bands / sums")
        sums = []
        if d.get("sums") is not None:
            if not isinstance(d["sums"], list):
                raise ValueError(f"{where}: features.sums must be a list of objects")
            for e in d["sums"]:
                if not isinstance(e, dict) or set(e) - {"coef", "lo", "hi", "k", "reduce"} or "coef" not in e:
                    raise ValueError(f"{where}: a sum is an object with the keys coef (and lo, hi, k, reduce)")
                sums.append(FeatureSum(e["coef"], e.get("lo"), e.get("hi"), e.get("k", 1.0), e.get("reduce", "sum")))
        b = d.get("bands")
        if b is None:
            return cls(sums=sums)
        if not isinstance(b, dict) or (set(b) - {"lo", "hi", "k"} and set(b) - {"target", "tol", "k"}):
            raise ValueError(f"{where}: features.bands holds the keys lo, hi, k or target, tol, k")
        if "target" in b:
            return cls.target(b["target"], b.get("k", 1.0), b.get("tol", 0.0), sums)
        return cls(b.get("lo"), b.get("hi"), b.get("k", 1.0), sums)

    def to_dict(self) -> dict:
        """The JSON form `from_dict` reads (None for an infinite bound)."""
        fin = lambda t: [fin(r) for r in t] if isinstance(t, list) else (t if math.isfinite(t) else None)
        out = {}
        if self.lo is not None:
            sq = lambda t: (t[0] if t.shape[0] == 1 else t).tolist()
            out["bands"] = {"lo": fin(sq(self.lo)), "hi": fin(sq(self.hi)), "k": sq(self.k)}
        if self.sums:
            one = lambda t: fin(t.tolist()[0] if t.numel() == 1 else t.tolist())
            out["sums"] = [{"coef": r.coef.tolist(), "lo": one(r.lo), "hi": one(r.hi), "k": r.k, "reduce": r.reduce} for r in self.sums]
        return out


def feature_ratio(schedule, nv0: float, nv1: float) -> float:
    """lambda^h_k / lambda_k: nv1 / nv0 under the "score" schedule (dv / dz_h = nv1 / alpha_t where dx / dz_x = nv0 / alpha_t), 1 for
    "sigma" and for explicit weights."""
    return float(nv1) / float(nv0) if isinstance(schedule, str) and schedule == "score" else 1.0


class Restraints:
    """The three tables of one call, validated and kept on the CPU.

    obstacles  [P, 5] or [B, P, 5]   rows (y_x, y_y, y_z, r, k); a row with r <= 0 or k <= 0 is padding
    pairs      [Q, 5] or [B, Q, 5]   rows (i, j, lo, hi, k); i = j = -1 is padding
    anchors    [A, 6] or [B, A, 6]   rows (i, a_x, a_y, a_z, r, k); i = -1 is padding
    fields     a `Field` or a list of at most MAX_FIELDS of them (lattice potentials; `field_energy`, not a column of `energy`)
    templates  a `Template` or a list of at most MAX_TEMPLATES of them (rigid superposition; `template_energy`)
    features   a `Features`: bands and molecule-wide sums on the features h (`feature_energy`)
    Tensors or nested lists; a table with a leading batch axis holds one set of rows per molecule.  ValueError: lo > hi, a negative
    r, k, lo or hi, non-finite values, i == j, fractional indices, negative indices other than -1."""

    def __init__(self, obstacles=None, pairs=None, anchors=None, fields=None, templates=None, features=None):
        if features is not None and not isinstance(features, Features):
            raise ValueError(f"features must be a restraints.Features, got {type(features).__name__}")
        self.features = features
        self.fields = _fields(fields)
        self.templates = _templates(templates)
        obs, pr, an = _table(obstacles, 5, "obstacles"), _table(pairs, 5, "pairs"), _table(anchors, 6, "anchors")
        if obs is not None and bool((obs[..., 3:] < 0).any()):
            raise ValueError("obstacles: r and k must be >= 0 (a row with r = 0 or k = 0 is padding)")
        self.obs = torch.zeros(1, 0, 5) if obs is None else obs.to(torch.float32).contiguous()
        self.pair_idx, self.pair_f = self._split(pr, 2, "pairs")
        self.anc_idx, self.anc_f = self._split(an, 1, "anchors")
        if pr is not None:
            live = self.pair_idx[..., 0] >= 0
            if bool(((self.pair_idx[..., 0] == self.pair_idx[..., 1]) & live).any()):
                raise ValueError("pairs: i == j")
            if bool(((self.pair_idx < 0).any(-1) & ~(self.pair_idx == -1).all(-1)).any()):
                raise ValueError("pairs: a padding row has i = j = -1")
            if bool((self.pair_f < 0).any()):
                raise ValueError("pairs: lo, hi and k must be >= 0")
            if bool((self.pair_f[..., 0] > self.pair_f[..., 1]).any()):
                raise ValueError("pairs: lo > hi")
        if an is not None and bool((self.anc_f[..., 3:] < 0).any()):
            raise ValueError("anchors: r and k must be >= 0")
        self.anc_idx = self.anc_idx[..., 0].contiguous()
        self._model = None                       # weak reference to the last model these restraints ran in (`energy` on a device)

    @staticmethod
    def _split(t, n_idx: int, name: str):
        if t is None:
            return torch.full((1, 0, n_idx), -1, dtype=torch.int32), torch.zeros(1, 0, 3 if n_idx == 2 else 5)
        idx = t[..., :n_idx]
        if bool((idx != idx.round()).any()) or bool((idx < -1).any()):
            raise ValueError(f"{name}: node indices must be integers >= 0, or -1 for padding")
        return idx.to(torch.int32).contiguous(), t[..., n_idx:].to(torch.float32).contiguous()

    @property
    def sizes(self):
        return int(self.obs.shape[1]), int(self.pair_idx.shape[1]), int(self.anc_idx.shape[1])

    def rows(self):
        return int(self.obs.shape[0]), int(self.pair_idx.shape[0]), int(self.anc_idx.shape[0])

    @property
    def n_fields(self) -> int:
        return len(getattr(self, "fields", ()))

    def field_rows(self) -> int:
        """Rows of the field weights: 1 (shared) or the B of the per-molecule ones."""
        return max([f.rows for f in getattr(self, "fields", ())] + [1])

    def field_weights(self, N: int) -> torch.Tensor:
        """[w_rows, NF, N] float32, always materialised: the library's weights."""
        r = self.field_rows()
        return torch.stack([f.node_weights(N).expand(r, N) for f in self.fields], 1).contiguous()

    @property
    def n_templates(self) -> int:
        return len(getattr(self, "templates", ()))

    def template_rows(self) -> int:
        """Rows of the template tables: 1 (shared) or the B of the per-molecule ones."""
        return max([t.rows for t in getattr(self, "templates", ())] + [1])

    def template_tables(self):
        """(idx [rows, NT, M] int32, f [rows, NT, M, 4] float32 = (y, w), geom [NT, 2] float32 = (k, fit)): the library's tables, M the
        longest template's, shorter ones padded with inactive rows (index -1, w = 0)."""
        tl = self.templates
        r, NT, M = self.template_rows(), len(tl), max(t.M for t in tl)
        idx = torch.full((r, NT, M), -1, dtype=torch.int32)
        f = torch.zeros((r, NT, M, 4), dtype=torch.float32)
        for j, t in enumerate(tl):
            idx[:, j, :t.M] = t.index
            f[:, j, :t.M, :3] = t.positions
            f[:, j, :t.M, 3] = t.weights
        geom = torch.tensor([[t.k, float(FITS.index(t.fit))] for t in tl], dtype=torch.float32)
        return idx.contiguous(), f.contiguous(), geom.contiguous()

    @property
    def feature_sizes(self):
        """(W, S) of the attached features, (0, 0) without."""
        ft = getattr(self, "features", None)
        return (0, 0) if ft is None else (ft.W, ft.S)

    def feature_rows(self):
        """(rows of the bands, rows of the sums): 1 (shared) or the B of the per-molecule ones."""
        ft = getattr(self, "features", None)
        return (1, 1) if ft is None else (ft.band_rows(), ft.sum_rows())

    def check_batch(self, B: int, what: str = "restraints") -> None:
        for name, r in zip(("obstacles", "pairs", "anchors", "field weights", "templates", "feature bands", "feature sums"),
                           self.rows() + (self.field_rows(), self.template_rows()) + self.feature_rows()):
            if r != 1 and r != int(B):
                raise ValueError(f"{what}: {name} hold rows for {r} molecules, the call has {B} (give [n, w] to share one set)")

    def slice(self, lo: int, hi: int) -> "Restraints":
        """The rows of molecules lo .. hi - 1 (shared tables stay shared)."""
        out = object.__new__(Restraints)
        for k in ("obs", "pair_idx", "pair_f", "anc_idx", "anc_f"):
            t = getattr(self, k)
            setattr(out, k, t if t.shape[0] == 1 else t[lo:hi].contiguous())
        out.fields = [f._slice(lo, hi) for f in getattr(self, "fields", ())]
        out.templates = [t._slice(lo, hi) for t in getattr(self, "templates", ())]
        ft = getattr(self, "features", None)
        out.features = None if ft is None else ft._slice(lo, hi)
        out._feat = getattr(self, "_feat", None)
        out._model = getattr(self, "_model", None)
        return out

    @classmethod
    def from_json(cls, path: str) -> "Restraints":
        """A JSON file with the keys `obstacles`, `pairs`, `anchors` (each optional; the row formats above) and `fields` (optional):
        a list of {"file": "pocket.npy", "origin": [...], "spacing": s | [...], "k": ..., "wall": ..., "weights": [...]} - `file`
        relative to the JSON file, read with numpy.load(allow_pickle=False); k, wall and weights optional - and `templates` (optional):
        a list of {"index": [...], "positions": [[...]], "weights": [...], "k": ..., "fit": "rigid" | "translation"}; weights, k and
        fit optional - and `features` (optional): {"bands": {"lo": ..., "hi": ..., "k": ...} | {"target": ..., "tol": ..., "k": ...},
        "sums": [{"coef": [...], "lo": ..., "hi": ..., "k": ..., "reduce": "sum" | "mean"}]}; null for an infinite bound."""
        import json
        import os
        with open(path) as f:
            d = json.load(f)
        if not isinstance(d, dict) or set(d) - {"obstacles", "pairs", "anchors", "fields", "templates", "features"}:
            raise ValueError(f"{path}: expected an object with the keys obstacles / pairs / anchors / fields / templates / features")
        features = None if d.get("features") is None else Features.from_dict(d["features"], path)
        templates = None
        if d.get("templates") is not None:
            if not isinstance(d["templates"], list):
                raise ValueError(f"{path}: templates must be a list of objects")
            templates = []
            for e in d["templates"]:
                if not isinstance(e, dict) or set(e) - {"index", "positions", "weights", "k", "fit"} or not {"index", "positions"} <= set(e):
                    raise ValueError(f"{path}: a template is an object with the keys index, positions (and weights, k, fit)")
                templates.append(Template(e["index"], e["positions"], e.get("weights"), e.get("k", 1.0), e.get("fit", "rigid")))
        fields = None
        if d.get("fields") is not None:
            if not isinstance(d["fields"], list):
                raise ValueError(f"{path}: fields must be a list of objects")
            fields = []
            for e in d["fields"]:
                if not isinstance(e, dict) or set(e) - {"file", "origin", "spacing", "k", "wall", "weights"} or \
                        not {"file", "origin", "spacing"} <= set(e) or not isinstance(e["file"], str):
                    raise ValueError(f"{path}: a field is an object with the keys file, origin, spacing (and k, wall, weights)")
                fn = os.path.join(os.path.dirname(os.path.abspath(path)), e["file"])
                try:
                    vals = np.load(fn, allow_pickle=False)
                except (OSError, ValueError) as err:
                    raise ValueError(f"{path}: cannot read the field file {e['file']!r}: {err}") from None
                fields.append(Field(vals, e["origin"], e["spacing"], e.get("k", 1.0), e.get("wall", 0.0), e.get("weights")))
        return cls(d.get("obstacles"), d.get("pairs"), d.get("anchors"), fields, templates, features)

    # ------------------------------------------------------------------ device side
    def attach(self, topo, scale: torch.Tensor, nv0: float, dev, stream, frame: int = 0, feat=None) -> None:
        """hd_restraint_attach: the tables and the scales [1] or [B] into the topology's buffers (stream-ordered copies).  `frame` 1:
        then hd_restraint_frame - the tables are in the frame of an inpainting call's known fragments (attaching resets to 0).  With
        fields, hd_restraint_fields goes between the two (attaching resets to no fields); `topo` then also needs its `.N`.  `feat`:
        (nv1, nb1, ratio) of the model and the resolved schedule - with it the features, if any, are attached too
        (hd_restraint_features; attaching resets to no features); without it the call sees none."""
        from . import _lib
        P, Q, A = self.sizes
        t = [x.to(dev).contiguous() for x in (self.obs, self.pair_idx, self.pair_f, self.anc_idx, self.anc_f, scale.to(torch.float32))]
        ro, rp, ra = self.rows()
        _lib.check(_lib.load().hd_restraint_attach(
            topo.ptr, t[0].data_ptr() if P else None, ro, P, t[1].data_ptr() if Q else None, t[2].data_ptr() if Q else None, rp, Q,
            t[3].data_ptr() if A else None, t[4].data_ptr() if A else None, ra, A, t[5].data_ptr(), int(t[5].numel()), float(nv0),
            stream), "hd_restraint_attach")
        if self.n_fields:                                # (attaching resets to no fields: the order is attach -> fields -> frame)
            self._attach_fields(topo, dev, stream)
        if self.n_templates:                             # (attaching resets to no templates; fields and templates in either order)
            self._attach_templates(topo, stream)
        if feat is not None and getattr(self, "features", None) is not None:
            self._attach_features(topo, feat, stream)
        if frame:
            _lib.check(_lib.load().hd_restraint_frame(topo.ptr, int(frame)), "hd_restraint_frame")

    def _attach_features(self, topo, feat, stream) -> None:
        """hd_restraint_features: the band tables and the sum rows (host arrays) into the topology's buffers; `feat` is remembered so
        that `feature_energy` on the call's result attaches the same and the cached graph stays."""
        import ctypes as C
        from . import _lib
        lo, hi, k, coef, f = (t.numpy() for t in self.features.tables())
        W, S = self.features.W, self.features.S
        fp = lambda a, n: a.ctypes.data_as(C.POINTER(C.c_float)) if n else None
        nv1, nb1, ratio = (float(v) for v in feat)
        _lib.check(_lib.load().hd_restraint_features(
            topo.ptr, fp(lo, W), fp(hi, W), fp(k, W), int(lo.shape[0]), W, fp(coef, S), fp(f, S), int(coef.shape[0]), S,
            nv1, nb1, ratio, stream), "hd_restraint_features")
        self._feat = (nv1, nb1, ratio)

    def _attach_fields(self, topo, dev, stream) -> None:
        """hd_restraint_fields: the lattices (each field's device copy; several are concatenated on the device), their geometry and
        the weights [w_rows, NF, N] into the topology's buffers."""
        import ctypes as C
        from . import _lib
        fl = self.fields
        NF = len(fl)
        vals = [f.device_values(dev) for f in fl]
        pool = vals[0].reshape(-1) if NF == 1 else torch.cat([v.reshape(-1) for v in vals])
        off = np.zeros(NF + 1, dtype=np.int64)
        off[1:] = np.cumsum([int(f.values.numel()) for f in fl])
        dims = np.ascontiguousarray([list(f.values.shape) for f in fl], dtype=np.int32)
        geom = np.ascontiguousarray(torch.stack([f.geom() for f in fl]).numpy(), dtype=np.float32)
        w = self.field_weights(int(topo.N)).to(dev).contiguous()
        _lib.check(_lib.load().hd_restraint_fields(
            topo.ptr, NF, pool.data_ptr(), off.ctypes.data_as(C.POINTER(C.c_longlong)), dims.ctypes.data_as(C.POINTER(C.c_int)),
            geom.ctypes.data_as(C.POINTER(C.c_float)), w.data_ptr(), int(w.shape[0]), stream), "hd_restraint_fields")

    def _attach_templates(self, topo, stream) -> None:
        """hd_restraint_templates: the row tables [rows, NT, M] and the geometry (host arrays) into the topology's buffers."""
        import ctypes as C
        from . import _lib
        idx, f, geom = (t.numpy() for t in self.template_tables())
        _lib.check(_lib.load().hd_restraint_templates(
            topo.ptr, int(idx.shape[1]), int(idx.shape[0]), int(idx.shape[2]), idx.ctypes.data_as(C.POINTER(C.c_int)),
            f.ctypes.data_as(C.POINTER(C.c_float)), geom.ctypes.data_as(C.POINTER(C.c_float)), stream), "hd_restraint_templates")

    @staticmethod
    def _framed_args(fixed_mask, x_known, B: int, N: int, dev, what: str):
        """None for a call in the model's frame, else (fixed_mask, x_known) after their checks; with a device `dev`, as the library
        takes them: uint8 [B * N] and float32 [B, N, 3] there."""
        if (fixed_mask is None) != (x_known is None):
            raise ValueError(f"{what}: fixed_mask and x_known go together")
        if fixed_mask is None:
            return None
        if fixed_mask.numel() != B * N or tuple(x_known.shape) != (B, N, 3):
            raise ValueError(f"{what}: fixed_mask must hold {B} x {N} entries and x_known be [{B}, {N}, 3]")
        if dev is None:
            return fixed_mask, x_known
        return (fixed_mask.to(dev).reshape(B * N) != 0).to(torch.uint8).contiguous(), x_known.detach().to(dev, torch.float32).contiguous()

    @staticmethod
    def _batch_shape(x, node_mask):
        B, N = int(node_mask.shape[0]), int(node_mask.shape[1])
        if tuple(x.shape) != (B, N, 3):
            raise ValueError(f"x must be [{B}, {N}, 3], got {tuple(x.shape)}")
        return B, N

    def _on_device(self, x, node_mask, model, _attach, what: str, call, features: bool = False):
        """The device path of `energy`, `field_energy` and `template_energy`, behind their checks: call(run) between attach and detach,
        where run(name, *args) is the library's entry point `name`(handle, topology, x as contiguous float32, *args, stream).
        (`_attach`: the scales and nv0 of the sampling call whose result this is - the energies read neither, and attaching what the
        call attached keeps its cached graph.)  `features`: the entry point reads the features - they are attached with what the last
        sampling call attached them with, or (1, 0, 1): the energies read h in data units, so neither enters."""
        model = model if model is not None else (self._model() if getattr(self, "_model", None) is not None else None)
        if model is None:
            raise ValueError(f"{what} on a device needs model= (the DiffusionQM9 that owns the library handle) unless these "
                             "restraints have already run in one of its sampling calls")
        from . import _lib
        from .dynamics import _stream
        dev = x.device
        h, stream = model._lib_handle(), _stream(dev)
        topo = model.dynamics.topology(node_mask.to(dev), None, int(node_mask.shape[0]), int(node_mask.shape[1]))
        xs = x.detach().to(torch.float32).contiguous()
        scale, nv0 = (torch.ones(1), 1.0) if _attach is None else _attach
        self.attach(topo, scale, nv0, dev, stream, feat=(getattr(self, "_feat", None) or (1.0, 0.0, 1.0)) if features else None)
        try:
            return call(lambda name, *args: _lib.check(getattr(_lib.load(), name)(h, topo.ptr, xs.data_ptr(), *args, stream), name))
        finally:
            self.detach(topo)

    def template_energy(self, x: torch.Tensor, node_mask: torch.Tensor, model=None, _attach=None):
        """(U [B, NT], fit [B, NT, 16]) float64 of positions x [B, N, 3] in data units under node_mask [B, N, 1]: U_tpl per template and
        its fit (R row-major [9], c_x [3], c_y [3], rmsd) - `template_frame` applies one.  On a device the HIP kernel evaluates it
        (k_restraint_template_energy; `model` as in `energy`); on the CPU the same formulas in torch float64.  Needs templates."""
        B, _ = self._batch_shape(x, node_mask)
        if not self.n_templates:
            raise ValueError("template_energy: these restraints hold no templates")
        self.check_batch(B, "template_energy")
        if x.device.type != "cuda":
            return template_energy_terms(self, x.detach().double(), node_mask, return_fit=True)

        def call(run):
            out = torch.empty((B, self.n_templates), device=x.device, dtype=torch.float64)
            fit = torch.empty((B, self.n_templates, 16), device=x.device, dtype=torch.float64)
            run("hd_restraint_template_energy", out.data_ptr(), fit.data_ptr())
            return out, fit

        return self._on_device(x, node_mask, model, _attach, "template_energy", call)

    def template_results(self, x: torch.Tensor, node_mask: torch.Tensor, model=None, _attach=None) -> dict:
        """The result entries of a templated call for its returned x: 'restraint_template_energy' [B, NT], 'template_rmsd' [B, NT] and
        'x_template_frame' [B, N, 3] = R_0^T (x - c_x) + c_y of template 0 (masked nodes 0), all float64 on x's device."""
        U, fit = self.template_energy(x, node_mask, model=model, _attach=_attach)
        B, N = int(node_mask.shape[0]), int(node_mask.shape[1])
        xt = template_frame(x, fit[:, 0]) * node_mask.reshape(B, N, 1).to(fit.device, torch.float64)
        return {'restraint_template_energy': U, 'template_rmsd': fit[..., 15].clone(), 'x_template_frame': xt}

    def field_energy(self, x: torch.Tensor, node_mask: torch.Tensor, model=None, fixed_mask=None, x_known=None, _attach=None):
        """[B] float64 U_fld of positions x [B, N, 3] in data units under node_mask [B, N, 1] (0 without fields).  On a device the HIP
        kernel evaluates it (k_restraint_field_energy; `model` as in `energy`); on the CPU the same formulas in torch float64.
        fixed_mask and x_known (together): in the frame of `x_known`, as `energy`."""
        B, N = self._batch_shape(x, node_mask)
        on_cpu = x.device.type != "cuda"
        framed = self._framed_args(fixed_mask, x_known, B, N, None if on_cpu else x.device, "field_energy")
        self.check_batch(B, "field_energy")
        if on_cpu:
            xd = x.detach().double()
            if framed:
                xd = xd - frame_shift(x, node_mask, *framed)[:, None, :]
            return field_energy_terms(self, xd, node_mask)

        def call(run):
            out = torch.empty((B,), device=x.device, dtype=torch.float64)
            if framed:
                run("hd_restraint_field_energy_framed", framed[0].data_ptr(), framed[1].data_ptr(), out.data_ptr(), None)
            else:
                run("hd_restraint_field_energy", out.data_ptr())
            return out

        return self._on_device(x, node_mask, model, _attach, "field_energy", call)

    def feature_energy(self, h: torch.Tensor, node_mask: torch.Tensor, model=None, _attach=None, return_sums: bool = False):
        """[B, 2] float64 (U_band, U_sum) of features h [B, N, F] in data units under node_mask [B, N, 1]; `return_sums`: (U, m [B, S]),
        m_r = 0 for a row that is inactive or contributes nothing.  On a device the HIP kernel evaluates it
        (k_restraint_feature_energy; `model` as in `energy`); on the CPU the same formulas in torch float64.  Needs features."""
        ft = getattr(self, "features", None)
        if ft is None:
            raise ValueError("feature_energy: these restraints hold no features")
        B, N = int(node_mask.shape[0]), int(node_mask.shape[1])
        if tuple(h.shape) != (B, N, ft.F):
            raise ValueError(f"h must be [{B}, {N}, {ft.F}], got {tuple(h.shape)}")
        if ft.W > N:
            raise ValueError(f"feature_energy: the bands name {ft.W} nodes, the molecules have {N}")
        self.check_batch(B, "feature_energy")
        if h.device.type != "cuda":
            U, m = feature_energy_terms(self, h.detach().double(), node_mask)
            return (U, m) if return_sums else U

        def call(run):
            out = torch.empty((B, 2), device=h.device, dtype=torch.float64)
            m = torch.zeros((B, ft.S), device=h.device, dtype=torch.float64)
            run("hd_restraint_feature_energy", out.data_ptr(), m.data_ptr() if ft.S else None)
            return (out, m) if return_sums else out

        return self._on_device(h, node_mask, model, _attach, "feature_energy", call, features=True)

    @staticmethod
    def detach(topo) -> None:
        from . import _lib
        _lib.check(_lib.load().hd_restraint_detach(topo.ptr), "hd_restraint_detach")

    def energy(self, x: torch.Tensor, node_mask: torch.Tensor, model=None, _attach=None, fixed_mask=None, x_known=None,
               return_shift: bool = False):
        """[B, 3] float64 (U_obs, U_pair, U_anc) of positions x [B, N, 3] in data units under node_mask [B, N, 1].  On a device the HIP
        kernel evaluates it (k_restraint_energy; `model`: the DiffusionQM9 whose handle and topology cache are used); on the CPU the
        same formulas in torch float64.  fixed_mask [B, N, 1] and x_known [B, N, 3] (together): the tables are in the frame of
        `x_known` - the energy of x - tau, tau = mean_F(x) - mean_F(x_known) over the valid fixed nodes (k_restraint_energy<true>);
        `return_shift`: (U, tau [B, 3] float64)."""
        B, N = self._batch_shape(x, node_mask)
        on_cpu = x.device.type != "cuda"
        framed = self._framed_args(fixed_mask, x_known, B, N, None if on_cpu else x.device, "energy")
        if return_shift and not framed:
            raise ValueError("energy: return_shift needs fixed_mask and x_known")
        self.check_batch(B, "energy")
        if on_cpu:
            if not framed:
                return energy_terms(self, x.detach().double(), node_mask)
            tau = frame_shift(x, node_mask, *framed)
            U = energy_terms(self, x.detach().double() - tau[:, None, :], node_mask)
            return (U, tau) if return_shift else U

        def call(run):
            out = torch.empty((B, 3), device=x.device, dtype=torch.float64)
            if not framed:
                run("hd_restraint_energy", out.data_ptr())
                return out
            tau = torch.empty_like(out)
            run("hd_restraint_energy_framed", framed[0].data_ptr(), framed[1].data_ptr(), out.data_ptr(), tau.data_ptr())
            return (out, tau) if return_shift else out

        return self._on_device(x, node_mask, model, _attach, "energy", call)

    def result_entries(self, x: torch.Tensor, node_mask: torch.Tensor, model, attach, fixed_mask=None, x_known=None, h=None) -> dict:
        """The restraint entries of a sampling call's results for its returned x, batch tensors on x's device: 'restraint_energy'
        [B, 3]; with fields 'restraint_field_energy' [B]; with templates the entries of `template_results`; for a call in the frame
        of `x_known` (fixed_mask, x_known) also 'frame_shift' [B, 3]; with features and the returned `h` [B, N, F] (data units)
        'restraint_feature_energy' [B, 2] and 'feature_sums' [B, S].  `attach`: the (scales, nv0) the call attached."""
        kw = dict(model=model, _attach=attach)
        framed = dict(fixed_mask=fixed_mask, x_known=x_known)
        if fixed_mask is None:
            out = {'restraint_energy': self.energy(x, node_mask, **kw)}
        else:
            out = dict(zip(('restraint_energy', 'frame_shift'), self.energy(x, node_mask, return_shift=True, **kw, **framed)))
        if self.n_fields:
            out['restraint_field_energy'] = self.field_energy(x, node_mask, **kw, **framed)
        if self.n_templates:
            out.update(self.template_results(x, node_mask, **kw))
        if getattr(self, "features", None) is not None and h is not None:
            U, m = self.feature_energy(h.to(x.device), node_mask, return_sums=True, **kw)
            out['restraint_feature_energy'], out['feature_sums'] = U, m
        return out


def energy_terms(rs: Restraints, x: torch.Tensor, node_mask: torch.Tensor) -> torch.Tensor:
    """[B, 3] (U_obs, U_pair, U_anc) in x's dtype, differentiable in x: the formulas of the module docstring in torch."""
    B, N = int(x.shape[0]), int(x.shape[1])
    nm = node_mask.reshape(B, N).bool().to(x.device)
    out = []
    for b in range(B):
        xb, m = x[b], nm[b]
        zero = xb.sum() * 0
        o = rs.obs[0 if rs.obs.shape[0] == 1 else b].to(x)
        o = o[(o[:, 3] > 0) & (o[:, 4] > 0)]
        u_obs = zero
        if o.shape[0] and bool(m.any()):
            d = _norm(xb[m][:, None, :] - o[None, :, :3])
            u_obs = 0.5 * (o[None, :, 4] * torch.clamp(o[None, :, 3] - d, min=0) ** 2).sum()
        pi = rs.pair_idx[0 if rs.pair_idx.shape[0] == 1 else b].long()
        pf = rs.pair_f[0 if rs.pair_f.shape[0] == 1 else b].to(x)
        u_pair = zero
        ok = (pi >= 0).all(1) & (pi < N).all(1) & (pi[:, 0] != pi[:, 1]) & (pf[:, 2] > 0)
        ok = ok & m[pi[:, 0].clamp(0, N - 1)] & m[pi[:, 1].clamp(0, N - 1)]
        if bool(ok.any()):
            pi, pf = pi[ok], pf[ok]
            d = _norm(xb[pi[:, 0]] - xb[pi[:, 1]])
            u_pair = 0.5 * (pf[:, 2] * (torch.clamp(d - pf[:, 1], min=0) ** 2 + torch.clamp(pf[:, 0] - d, min=0) ** 2)).sum()
        ai = rs.anc_idx[0 if rs.anc_idx.shape[0] == 1 else b].long()
        af = rs.anc_f[0 if rs.anc_f.shape[0] == 1 else b].to(x)
        u_anc = zero
        ok = (ai >= 0) & (ai < N) & (af[:, 4] > 0)
        ok = ok & m[ai.clamp(0, N - 1)]
        if bool(ok.any()):
            ai, af = ai[ok], af[ok]
            d = _norm(xb[ai] - af[:, :3])
            u_anc = 0.5 * (af[:, 4] * torch.clamp(d - af[:, 3], min=0) ** 2).sum()
        out.append(torch.stack([u_obs, u_pair, u_anc]))
    return torch.stack(out)


def field_energy_terms(rs: Restraints, x: torch.Tensor, node_mask: torch.Tensor) -> torch.Tensor:
    """[B] U_fld in x's dtype, differentiable in x: the field formulas of the module docstring in torch (x already in the fields'
    frame).  A node with a non-finite coordinate contributes nothing."""
    B, N = int(x.shape[0]), int(x.shape[1])
    nm = node_mask.reshape(B, N).bool().to(x.device)
    total = torch.zeros(B, dtype=x.dtype, device=x.device)
    for f in getattr(rs, "fields", ()):
        w = f.node_weights(N).to(x)
        w = w.expand(B, N) if w.shape[0] == 1 else w
        ok = nm & torch.isfinite(x).all(-1)
        xs = torch.where(ok[..., None], x, torch.zeros_like(x))
        o, h = f.origin.to(x), f.spacing.to(x)
        n = torch.tensor(list(f.values.shape), device=x.device)
        u = (xs - o) / h
        ub = torch.minimum(torch.clamp(u, min=0), (n - 1).to(x))
        cell = torch.minimum(torch.floor(ub.detach()).long(), n - 2)
        t = ub - cell.to(x)
        v = f.values.to(x)
        V = 0
        for a in (0, 1):
            for b in (0, 1):
                for c in (0, 1):
                    wa = t[..., 0] if a else 1 - t[..., 0]
                    wb = t[..., 1] if b else 1 - t[..., 1]
                    wc = t[..., 2] if c else 1 - t[..., 2]
                    V = V + v[cell[..., 0] + a, cell[..., 1] + b, cell[..., 2] + c] * wa * wb * wc
        out = (u - ub) * h
        e = f.k * w * (V + 0.5 * f.wall * (out * out).sum(-1))
        total = total + torch.where(ok, e, torch.zeros_like(e)).sum(1)
    return total


def feature_energy_terms(rs: Restraints, h: torch.Tensor, node_mask: torch.Tensor):
    """([B, 2] (U_band, U_sum), m [B, S]) in h's dtype, differentiable in h: the feature formulas of the module docstring in torch.
    A non-finite element has no band term; a sum row that reads one contributes nothing (m_r = 0)."""
    ft = rs.features
    B, N, F = int(h.shape[0]), int(h.shape[1]), int(h.shape[2])
    nm = node_mask.reshape(B, N).bool().to(h.device)
    fin = torch.isfinite(h)
    hs = torch.where(fin, h, torch.zeros_like(h))
    n = nm.sum(1).to(h)
    ub = h.new_zeros(B)
    if ft.W:
        W = min(ft.W, N)
        lo, hi, k = (t[:, :W].to(h).expand(B, W, F) for t in (ft.lo, ft.hi, ft.k))
        v = hs[:, :W]
        d = torch.clamp(v - hi, min=0) - torch.clamp(lo - v, min=0)
        act = nm[:, :W, None] & fin[:, :W] & (k > 0)
        ub = (0.5 * torch.where(act, k * d * d, torch.zeros_like(d))).sum((1, 2))
    us, ms = h.new_zeros(B), []
    for r in ft.sums:
        c = r.coef.to(h)
        read = nm[:, :, None] & (c != 0)[None, None, :]
        ok = ~(read & ~fin).any(2).any(1) & (n > 0) & (r.k > 0)
        s = torch.where(read, c * hs, torch.zeros_like(hs)).sum((1, 2))
        m = s / n.clamp(min=1.0) if r.reduce == "mean" else s
        m = torch.where(ok, m, torch.zeros_like(m))
        lo, hi = r.lo.to(h).expand(B), r.hi.to(h).expand(B)
        d = torch.clamp(m - hi, min=0) - torch.clamp(lo - m, min=0)
        us = us + torch.where(ok, 0.5 * r.k * d * d, torch.zeros_like(d))
        ms.append(m)
    return torch.stack([ub, us], 1), (torch.stack(ms, 1) if ms else h.new_zeros(B, 0))


def kabsch_rotation(S: torch.Tensor) -> torch.Tensor:
    """R [3, 3] = argmax over proper rotations of tr(R^T S) for S [3, 3] = sum w x' y'^T (x' ~ R y'): Horn's quaternion form, the
    eigenvector of the largest eigenvalue of the symmetric 4x4 matrix by torch.linalg.eigh.  Never a reflection."""
    xx, xy, xz, yx, yy, yz, zx, zy, zz = S.reshape(9).unbind()
    K = torch.stack([torch.stack([xx + yy + zz, zy - yz, xz - zx, yx - xy]),
                     torch.stack([zy - yz, xx - yy - zz, xy + yx, zx + xz]),
                     torch.stack([xz - zx, xy + yx, -xx + yy - zz, yz + zy]),
                     torch.stack([yx - xy, zx + xz, yz + zy, -xx - yy + zz])])
    q = torch.linalg.eigh(K)[1][:, -1]
    q0, q1, q2, q3 = (q / q.norm()).unbind()
    return torch.stack([torch.stack([q0 * q0 + q1 * q1 - q2 * q2 - q3 * q3, 2 * (q1 * q2 - q0 * q3), 2 * (q1 * q3 + q0 * q2)]),
                        torch.stack([2 * (q1 * q2 + q0 * q3), q0 * q0 - q1 * q1 + q2 * q2 - q3 * q3, 2 * (q2 * q3 - q0 * q1)]),
                        torch.stack([2 * (q1 * q3 - q0 * q2), 2 * (q2 * q3 + q0 * q1), q0 * q0 - q1 * q1 - q2 * q2 + q3 * q3])])


def template_energy_terms(rs: Restraints, x: torch.Tensor, node_mask: torch.Tensor, return_fit: bool = False):
    """[B, NT] U_tpl in x's dtype, differentiable in x: the template formulas of the module docstring in torch.  R is found under
    no_grad - it maximises, so autograd through the rest gives the exact gradient k w r.  `return_fit`: (U, fit [B, NT, 16]) with
    fit = (R row-major, c_x, c_y, rmsd), detached; a template that contributes nothing reports R = I, c_x = c_y = 0, rmsd = 0."""
    B, N = int(x.shape[0]), int(x.shape[1])
    nm = node_mask.reshape(B, N).bool().to(x.device)
    tl = getattr(rs, "templates", ())
    U, fits = [], torch.zeros(B, len(tl), 16, dtype=x.dtype, device=x.device)
    for b in range(B):
        row = []
        for j, t in enumerate(tl):
            r_ = 0 if t.rows == 1 else b
            idx, y, w = t.index[r_].long().to(x.device), t.positions[r_].to(x), t.weights[r_].to(x)
            act = (idx >= 0) & (idx < N) & (w > 0)
            act = act & nm[b][idx.clamp(0, N - 1)]
            fits[b, j, 0] = fits[b, j, 4] = fits[b, j, 8] = 1.0
            u = x.new_zeros(())
            if int(act.sum()) >= 2 and bool(torch.isfinite(x[b][idx[act]]).all()):
                xi, y, w = x[b][idx[act]], y[act], w[act]
                W = w.sum()
                cx, cy = (w[:, None] * xi).sum(0) / W, (w[:, None] * y).sum(0) / W
                xp, yp = xi - cx, y - cy
                with torch.no_grad():
                    R = kabsch_rotation((w[:, None, None] * xp[:, :, None] * yp[:, None, :]).sum(0)) if t.fit == "rigid" \
                        else torch.eye(3, dtype=x.dtype, device=x.device)
                res = xp - yp @ R.T
                q = (w * (res * res).sum(-1)).sum()
                u = 0.5 * t.k * q
                fits[b, j] = torch.cat([R.reshape(9), cx.detach(), cy, torch.sqrt(q.detach() / W).reshape(1)])
            row.append(u)
        U.append(torch.stack(row) if row else x.new_zeros(0))
    U = torch.stack(U)
    return (U, fits) if return_fit else U


def template_frame(x: torch.Tensor, fit: torch.Tensor) -> torch.Tensor:
    """x [..., N, 3] in the coordinates of a template: R^T (x - c_x) + c_y for fit [..., 16] (float64)."""
    fit = fit.to(torch.float64)
    R = fit[..., :9].reshape(fit.shape[:-1] + (3, 3))
    return (x.to(fit.device, torch.float64) - fit[..., None, 9:12]) @ R + fit[..., None, 12:15]


def entries_into(res: dict, entries: dict, i: int, n: int) -> None:
    """Molecule i (n nodes) of `Restraints.result_entries`, moved to the CPU (and a site's own per-node entries), into the result dict
    of that molecule."""
    for k, v in entries.items():
        res[k] = (v[i, :n] if k in ('x_template_frame', 'x_known_frame') else v[i]).clone()


def _norm(v):
    """|v| along the last axis with a zero (sub)gradient at v = 0."""
    s = (v * v).sum(-1)
    safe = torch.where(s > 0, s, torch.ones_like(s))
    return torch.where(s > 0, torch.sqrt(safe), torch.zeros_like(s))


# ----------------------------------------------------------------------------- the per-transition rows

def check_clip(clip) -> float:
    if clip is None:
        return math.inf
    if isinstance(clip, bool) or not isinstance(clip, (int, float, np.integer, np.floating)) or not float(clip) > 0.0:
        raise ValueError(f"restraint_clip must be a positive number (None or inf: no clip), got {clip!r}")
    return float(clip)


def lambda_rows(gamma, path: Sequence[int], schedule="score", clip=None, nv0: float = 1.0) -> np.ndarray:
    """[K, 4] float32 rows {alpha_t, sigma_t, lambda_k, clip_k} of the transitions of `path` (grid indices, path[k] -> path[k + 1];
    the departure level t = path[k] counts), from the gamma grid.  alpha_t / sigma_t are the fp32 sqrt(sigmoid(-+gamma_t)) of the fp32
    grid - the values `record="x0"` uses; lambda_k is evaluated in float64 and rounded once:
        "score" (default)   lambda_k = nv0 sigma_t / alpha_t   the score-guidance weight with d eps^ / d z ignored:
                            d x^0 / d z_x = nv0 / alpha_t, and a score s enters eps^ as -sigma_t s
        "sigma"             lambda_k = sigma_t
        a length-K sequence explicit weights
    clip: the largest |Delta_i| per node in eps units (None: no clip)."""
    g32 = torch.as_tensor(gamma).detach().to(torch.float32).reshape(-1)
    g64 = torch.as_tensor(gamma).detach().to(torch.float64).reshape(-1)
    K = len(path) - 1
    if K < 1:
        raise ValueError("lambda_rows: the path has no transition")
    c = check_clip(clip)
    t = torch.as_tensor(list(path[:-1]), dtype=torch.int64)
    al32, sg32 = torch.sqrt(torch.sigmoid(-g32[t])), torch.sqrt(torch.sigmoid(g32[t]))
    if isinstance(schedule, str):
        if schedule not in SCHEDULES:
            raise ValueError(f"restraint_schedule must be one of {SCHEDULES} or a length-K sequence, got {schedule!r}")
        al, sg = torch.sqrt(torch.sigmoid(-g64[t])), torch.sqrt(torch.sigmoid(g64[t]))
        lam = float(nv0) * sg / al if schedule == "score" else sg
    else:
        try:
            lam = torch.as_tensor(schedule, dtype=torch.float64).reshape(-1)
        except (TypeError, ValueError, RuntimeError):
            raise ValueError(f"restraint_schedule must be one of {SCHEDULES} or a length-K sequence, got {schedule!r}") from None
        if lam.numel() != K or not bool(torch.isfinite(lam).all()):
            raise ValueError(f"restraint_schedule: an explicit sequence holds one finite weight per transition ({K})")
    rows = np.empty((K, 4), dtype=np.float32)
    rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3] = al32.numpy(), sg32.numpy(), lam.numpy().astype(np.float32), np.float32(c)
    return rows


class Resolved:
    """A restrained call: the tables, the scales float32 [1] or [B] (CPU), the schedule and the clip."""

    def __init__(self, rs: Restraints, scale: torch.Tensor, schedule, clip: float, frame: int = 0):
        self.rs, self.scale, self.schedule, self.clip = rs, scale, schedule, clip
        self.frame = frame                       # 0: the model's frame; 1: the known fragments' (inpainting plans only)

    def key(self):
        s = self.schedule
        return (s if isinstance(s, str) else tuple(float(v) for v in torch.as_tensor(s).reshape(-1).tolist()), self.clip)


def resolve(model, restraints, scale, schedule, clip, B: Optional[int] = None, what: str = "restraints", pocket=None,
            needs_noise: bool = True, steered: bool = False) -> Optional[Resolved]:
    """Keywords (None: the model's `restraints` / `restraint_scale` / `restraint_schedule` / `restraint_clip`) -> None for the
    unrestrained code path, untouched, or a `Resolved`.  No restraints, or a scale of None or 0, is the unrestrained path.  Pure host
    checks: every error is raised before a device is looked at.  `steered`: the call steers particles by the restraint energy
    (hierdiff_amd/steering.py), which needs the tables but not the gradient update - a scale of None or 0 then resolves to a
    `Resolved` with the scale 0 (k_restrain_eps writes nothing)."""
    restraints = model.restraints if restraints is None else restraints
    scale = model.restraint_scale if scale is None else scale
    schedule = model.restraint_schedule if schedule is None else schedule
    clip = model.restraint_clip if clip is None else clip
    if restraints is None:
        return None
    if not isinstance(restraints, Restraints):
        raise ValueError(f"restraints must be a hierdiff_amd.restraints.Restraints, got {type(restraints).__name__}")
    if scale is None:
        if not steered:
            return None
        scale = 0.0
    if isinstance(scale, bool):
        raise ValueError(f"restraint_scale must be a number or a [B] tensor, got {scale!r}")
    try:
        s = torch.as_tensor(scale, dtype=torch.float32).detach().cpu()
    except (TypeError, ValueError, RuntimeError):
        raise ValueError(f"restraint_scale must be a number or a [B] tensor, got {scale!r}") from None
    s = s.reshape(1) if s.dim() == 0 else s
    if s.dim() != 1 or s.numel() < 1 or not bool(torch.isfinite(s).all()):
        raise ValueError("restraint_scale must be a finite number or a [B] tensor")
    if B is not None and s.numel() not in (1, int(B)):
        raise ValueError(f"restraint_scale must hold one scale per molecule ([{B}]), got {s.numel()}")
    if not isinstance(schedule, str):
        try:
            torch.as_tensor(schedule, dtype=torch.float64)
        except (TypeError, ValueError, RuntimeError):
            raise ValueError(f"restraint_schedule must be one of {SCHEDULES} or a length-K sequence, got {schedule!r}") from None
    elif schedule not in SCHEDULES:
        raise ValueError(f"restraint_schedule must be one of {SCHEDULES} or a length-K sequence, got {schedule!r}")
    c = check_clip(clip)
    if not bool((s != 0).any()) and not steered:
        return None
    ft = getattr(restraints, "features", None)
    if ft is not None and ft.F != int(model.in_node_nf):
        raise ValueError(f"{what}: the features name {ft.F} channels, the model's h has {int(model.in_node_nf)}")
    from .plan import unsupported
    unsupported(model, f"{what}: restraints", pocket, needs_noise)         # (the model's frame is the ligand's alone)
    if B is not None:
        restraints.check_batch(B, what)
    return Resolved(restraints, s.contiguous(), schedule, c)


def refuse(model, what: str, restraints=None, why: str = "") -> None:
    """Entry points that take no restraints: an error when the keyword or the model's attributes ask for them, instead of ignoring
    them."""
    if restraints is not None or resolve(model, None, None, None, None, None, what) is not None:
        raise NotImplementedError(f"{what}: restraints are not supported here{why} (the `restraints` keyword, or model.restraints "
                                  "with a non-zero model.restraint_scale); they act in sample / sample_from_masks / path_steps / "
                                  "sample_from_latent / vary")
