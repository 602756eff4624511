"""The host side of a sampling call: its keywords resolved once, before the GPU is touched.

Every sampling entry point of `hierdiff_amd/diffusion.py` takes the same keywords (`KEYWORDS`; None: the model's attribute of the
same meaning).  `plan` turns them into one immutable `Plan` - which loop runs (a path, or the plain every-step loop), with which
update, guided, restrained or recorded - by host arithmetic alone, so every argument error is raised before a device is looked at.
The entry points then build the device state (`DiffusionQM9._device_state`), run the transitions (`_run`) and decode (`_decode`)."""
from __future__ import annotations

from typing import List, NamedTuple, Optional

import numpy as np
import torch

from . import corrector as _corrector, diversity as _diversity, guidance as _guidance, paths, restraints as _rs, steering as _steering

#: the sampling keywords of the entry points; the list forms (`sample`, `sample_batches`, `vary`, the EDM signature) forward those given
KEYWORDS = ("steps", "eta", "spacing", "timesteps", "guidance_scale", "guidance_context", "guidance_rescale", "solver",
            "lower_order_final", "keep_frames", "record", "restraints", "restraint_scale", "restraint_schedule", "restraint_clip",
            "particles", "steer_scale", "steer_ess", "steer_schedule", "restraint_frame", "diversity", "corrector")


def given(values: dict) -> dict:
    """The sampling keywords of `values` (a call's locals, or its **kw) that are not None."""
    return {k: values[k] for k in KEYWORDS if values.get(k) is not None}


class Plan(NamedTuple):
    path: Optional[List[int]]                     # grid indices T .. 0 (t_start .. 0) of the path loop; None: the plain every-step loop
    eta: object                                   # the update on the path: eta in [0, 1], or the `paths.Multistep` of solver "dpm2m" / "sde2m"
    K: int                                        # transitions
    guidance: Optional[_guidance.Guidance]
    restraints: Optional[_rs.Resolved]
    frames: Optional[paths.ChainFrames]           # a recording call: frame of every transition; None: nothing is recorded
    record: Optional[int]                         # the library's code of `record`: 0 "z", 1 "x0"
    chain_t: Optional[torch.Tensor]               # [keep] int64, the grid index every frame has arrived at
    steer: Optional[_steering.Steer] = None       # a steered call: particles per group, beta, rho; None: the unsteered code path
    diversity: Optional[_diversity.Diversity] = None   # a diverse call: rows of a group repel by aligned RMSD; None: the code path without
    corrector: Optional[_corrector.Corrector] = None   # a corrected call: Langevin steps ahead of every predictor step; None: the code path without


def unsupported(model, what: str, pocket=None, needs_noise: bool = True, pocket_error=NotImplementedError) -> None:
    """The configurations the library's loops do not run: pocket models (whole molecules only), mode 'gnn_dynamics' (the loops
    evaluate the egnn network) and - when the call draws its own noise - noise_mode 'torch'.  `what`: the call and its feature.
    `pocket_error`: the editing entry points (`_edit_check`) raise ValueError for pocket models, as they always did; being one call,
    the check now comes after their shape, context and sample_id_base checks, where the pocket part used to come before them."""
    if model.pocket or pocket is not None:
        raise pocket_error(f"{what} is not supported for pocket models (whole molecules only)")
    if getattr(model.dynamics, "mode", "egnn_dynamics") == "gnn_dynamics":
        raise NotImplementedError(f"{what} runs inside the library's loop: mode 'gnn_dynamics' is not supported")
    if needs_noise and model.noise_mode == "torch":
        raise NotImplementedError(f"{what} runs inside the library's loop: noise_mode 'torch' is not supported (counter-based or "
                                  "injected noise only)")


def _spacing(model, spacing):
    spacing = model.sample_spacing if spacing is None else spacing
    if spacing not in paths.SPACINGS:
        raise ValueError(f"spacing must be one of {paths.SPACINGS}, got {spacing!r}")
    return spacing


def full_path(model, steps=None, eta=None, spacing=None, timesteps=None, inpaint: bool = False, solver=None, lower_order_final=None,
              force_path: bool = False):
    """The path keywords of a chain from T -> None for the plain loop, or (path, eta); with solver "dpm2m" (path, `paths.Multistep`)
    or "sde2m" - always the path loop, eta = 0 (1 with "sde2m") whatever `sample_eta` says.  `force_path` (or the model's `_force_path_loop`): also the identity
    path with ancestral steps, which IS the plain loop, comes back as a path."""
    force_path = force_path or model._force_path_loop
    if steps is None and timesteps is None:
        steps, timesteps = model.sample_steps, model.sample_timesteps
    ms = paths.check_solver(model.sample_solver if solver is None else solver, eta,
                            model.sample_lower_order_final if lower_order_final is None else lower_order_final)
    if ms is not None:
        if inpaint:
            raise ValueError(f"inpainting takes ancestral steps only (eta = 1), not solver '{'sde2m' if ms.stochastic else 'dpm2m'}': "
                             "the replacement method re-noises the known part with the posterior's own variance")
        return paths.build_path(model.T, steps, _spacing(model, spacing), timesteps), ms
    eta = paths.check_eta(model.sample_eta if eta is None else eta)
    spacing = _spacing(model, spacing)
    if steps is not None and timesteps is not None:
        raise ValueError("give either steps or timesteps, not both")
    if inpaint and eta < 1.0:
        raise ValueError("inpainting takes ancestral steps only (eta = 1): the replacement method re-noises the known part "
                         "with the posterior's own variance")
    if steps is None and timesteps is None and eta == 1.0 and not force_path:
        return None
    path = paths.build_path(model.T, steps, spacing, timesteps)
    if len(path) == model.T + 1 and eta == 1.0 and not force_path:
        return None
    return path, eta


def latent_path(model, t_start, steps, eta, spacing, timesteps, solver=None, lower_order_final=None):
    """(t_start, partial path, eta - or the `paths.Multistep` of solver "dpm2m") of a chain from `t_start` (None: T)."""
    t_start = model._grid_index(model.T if t_start is None else t_start, 1, "t_start")
    ms = paths.check_solver(model.sample_solver if solver is None else solver, eta,
                            model.sample_lower_order_final if lower_order_final is None else lower_order_final)
    eta = ms if ms is not None else paths.check_eta(model.sample_eta if eta is None else eta)
    spacing = model.sample_spacing if spacing is None else spacing
    return t_start, paths.partial_path(model.T, t_start, steps, spacing, timesteps), eta


def plan(model, what: str, kind: str = "full", *, t_start=None, pocket=None, injected: bool = False, B: Optional[int] = None,
         N: Optional[int] = None, force_path: bool = False, guided: bool = True, steps=None, eta=None, spacing=None, timesteps=None, guidance_scale=None,
         guidance_context=None, guidance_rescale=None, solver=None, lower_order_final=None, keep_frames=None, record=None,
         restraints=None, restraint_scale=None, restraint_schedule=None, restraint_clip=None,
         particles=None, steer_scale=None, steer_ess=None, steer_schedule=None, restraint_frame=None, diversity=None, corrector=None) -> Plan:
    """The `Plan` of the call `what`.  `kind`: "full" (the chain from T), "latent" (from `t_start`) or "inpaint" (from T, ancestral
    steps only; it takes restraints only with restraint_frame="known" - its callers refuse them otherwise - and then always runs on
    a path; "known" with restraints in any other kind is a ValueError).  `pocket`: the fixed residues of the call, if any; `injected`: the
    caller brings its own noise; `B` / `N`: the batch, where the caller knows it (shapes of per-molecule scales are checked);
    `force_path`: never the plain loop; `guided=False`: the call takes no guidance (`inpaint_steps`).

    particles / steer_scale / steer_ess / steer_schedule: steered sampling (hierdiff_amd/steering.py) -> `Plan.steer`; particles of
    None or 1, or a steer_scale of None or 0, is the unsteered plan, field for field.  Its errors come last, behind the chain's, so
    no earlier refusal moves; an inpainting plan refuses it.

    diversity: diverse sampling (hierdiff_amd/diversity.py) -> `Plan.diversity`; None, particles = 1, or a strength or scale of 0 is the
    plan without it, field for field.  Its errors come behind steering's; an inpainting plan and a steered plan refuse it.

    corrector: predictor-corrector sampling (hierdiff_amd/corrector.py) -> `Plan.corrector`; None, steps = 0, or a strength of 0 in every
    row is the plan without it, field for field.  Its errors come last, behind diversity's; an inpainting plan, a steered plan and a call
    with injected noise refuse it.

    Errors are raised in this order: path and solver, guidance, restraints, chain (keep_frames / record), steering, diversity, corrector; the
    shapes of a call's tensors are its entry point's business and come after the plan.  A guided, restrained, recorded, diverse or corrected call always runs on a path:
    where the keywords ask for the plain loop it gets the identity path with ancestral steps - here, and nowhere else."""
    if kind == "latent":
        _, path, eta = latent_path(model, t_start, steps, eta, spacing, timesteps, solver, lower_order_final)
    else:
        pe = full_path(model, steps, eta, spacing, timesteps, kind == "inpaint", solver, lower_order_final, force_path)
        path, eta = (None, 1.0) if pe is None else pe
    needs_noise = not injected
    gd = _guidance.resolve(model, guidance_scale, guidance_context, guidance_rescale, B, N, what, pocket, needs_noise) if guided else None
    rr = None
    steered = _steering.wanted(model, particles, steer_scale)
    frame = _rs.check_frame(model, restraint_frame)
    if kind != "inpaint":
        rr = _rs.resolve(model, restraints, restraint_scale, restraint_schedule, restraint_clip, B, what, pocket, needs_noise,
                         steered=steered)
        if rr is not None and frame:
            raise ValueError(f"{what}: restraint_frame='known' reads the tables in the frame of an inpainting call's known fragments; "
                             "it acts in sample_inpaint / sample_grow / inpaint_steps only")
    elif frame:
        rr = _rs.resolve(model, restraints, restraint_scale, restraint_schedule, restraint_clip, B, what, pocket, needs_noise)
        if rr is not None:
            rr.frame = frame
    code = None
    if keep_frames is None:
        if record is not None:
            raise ValueError(f"{what}: record={record!r} records nothing without keep_frames")
    else:
        if record not in (None, "z", "x0"):
            raise ValueError(f"{what}: record must be 'z' or 'x0', got {record!r}")
        if isinstance(keep_frames, bool) or not isinstance(keep_frames, (int, np.integer)):
            raise ValueError(f"{what}: keep_frames must be an integer, got {keep_frames!r}")
        unsupported(model, f"{what}: recording a chain", pocket, needs_noise)
        code = 1 if record == "x0" else 0
    diverse = _diversity.wanted(model, diversity)
    corrected = _corrector.wanted(model, corrector)
    if path is None and (gd is not None or rr is not None or code is not None or ((diverse or corrected) and kind != "inpaint")):
        path, eta = paths.build_path(model.T), 1.0
    frames = chain_t = None
    if code is not None:
        frames = paths.chain_frames(len(path) - 1, keep_frames, path)
        chain_t = torch.tensor(frames.frame_t, dtype=torch.int64)
    K = model.T if path is None else len(path) - 1
    st = None
    if steered:
        if kind == "inpaint":
            raise NotImplementedError(f"{what}: steered sampling is not supported here: inpainting takes no restraints (it acts in "
                                      f"{_steering.WHERE})")
        unsupported(model, f"{what}: steering", pocket, needs_noise)
        st = _steering.resolve(model, particles, steer_scale, steer_ess, steer_schedule, eta, K, rr is not None, B, what,
                               injected=injected)
    dv = None
    if diverse:
        if kind == "inpaint":
            raise NotImplementedError(f"{what}: diverse sampling is not supported here: inpainting re-centres on the known fragments "
                                      f"(it acts in {_diversity.WHERE})")
        unsupported(model, f"{what}: diversity", pocket, needs_noise)
        dv = _diversity.resolve(model, diversity, eta, K, B, what, injected=injected, steered=st is not None)
    cr = None
    if corrected:
        if kind == "inpaint":
            raise NotImplementedError(f"{what}: predictor-corrector sampling is not supported here: the replacement of the known fragments "
                                      f"would have to be redone behind every corrector step (it acts in {_corrector.WHERE})")
        if injected:
            raise NotImplementedError(f"{what}: predictor-corrector sampling takes no injected noise (raw_noises): its K + 2 rows hold none "
                                      "for the corrector steps (counter-based generator only)")
        unsupported(model, f"{what}: predictor-corrector sampling", pocket, True)
        cr = _corrector.resolve(model, corrector, K, what, steered=st is not None)
    return Plan(path, eta, K, gd, rr, frames, code, chain_t, st, dv, cr)
