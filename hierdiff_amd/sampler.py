"""Command-line sampler with the reference's wire format.

Replaces `endiffusion/sampler.py:24-41` without Hydra: build the model from the production hyper-parameters
(`conf/model/ddpmgblur.yaml`), load a reference Lightning checkpoint's `state_dict` (keys unchanged, a leading
`model.` prefix is stripped as the reference does, sampler.py:31-32), sample `batch_size x num_batches`
molecules and write `sample_results.pkl` = `pickle((results, test_names))` with
`results: list[{'x': FloatTensor[n,3], 'h': FloatTensor[n,8] (, 'context': FloatTensor[n,1])}]` — exactly what
`generation/ar_sampling_nosize.py:328-329` (`pickle.load(f)[0]`) consumes.

    python -m hierdiff_amd.sampler --checkpoint diffusion.ckpt --batch-size 256 --num-batches 4 --out sample_results.pkl

Fragment growing (no reference counterpart): `--known FILE --grow N [--resamplings R]` keeps the fragments of every molecule in
FILE (this sampler's own output: a list of {'x', 'h'}, pickled alone or as the (results, test_names) tuple, or saved with torch.save
as `.pt`) and samples N more around each (`DiffusionQM9.sample_grow`); the output format is unchanged, the known fragments come
first.  Single process only.  `--known-parts x|h|both` keeps only the positions or only the features of every entry: `--known lead.pkl
--known-parts h --grow 0` lays a lead's fragments out again, `--known-parts x --grow 0` re-assigns fragments to its positions.

Editing given molecules (no reference counterpart; mechanism only - which settings are chemically useful is for you to validate):
`--vary FILE --t-start S [--variants V]` noises every molecule of FILE to the grid index S and runs the reverse chain from there
(`DiffusionQM9.vary`; combines with --steps / --eta / --spacing / --solver, which then spread over the S steps below the start);
`--interpolate FILE --frames L` encodes consecutive molecules of FILE to their latents, interpolates on the sphere and decodes L
frames per pair (`DiffusionQM9.interpolate`; --steps / --spacing apply to both directions; pairs of unequal size are skipped with a
note).  Output: the same pickle format.  Single process only.

Multi-GPU: launch under `python -m torch.distributed.run --nproc-per-node N`; rank 0's weights are broadcast once,
each rank samples a contiguous share of the global sample ids and writes `<out>.rank<r>`; rank 0 concatenates
them in id order into `<out>`.
"""
from __future__ import annotations

import argparse
import math
import os
import pickle
from typing import Dict, List, Optional, Tuple

import torch

from .diffusion import DiffusionQM9, default_config
from .sharding import broadcast_model_weights, shard_sample_ids


def load_reference_state_dict(path: str, trust_checkpoint: bool = False) -> Dict[str, torch.Tensor]:
    """`torch.load(ckpt)['state_dict']` with the leading `model.` prefix removed (sampler.py:27-32).  Tensors that
    do not belong to the sampling half (optimizer state is not in `state_dict`; `pocket_embed.*` only exists for
    pocket models) are passed through untouched and rejected by load_state_dict if unexpected.

    The file is read with `weights_only=True` (tensors and plain containers only).  A Lightning checkpoint that
    carries pickled hyper-parameter objects needs the unrestricted unpickler, which executes code from the file:
    that path is taken only with `trust_checkpoint=True` (CLI: --trust-checkpoint)."""
    try:
        ckpt = torch.load(path, map_location="cpu", weights_only=True)
    except Exception as exc:
        if not trust_checkpoint:
            raise RuntimeError(f"{path}: not loadable with weights_only=True ({type(exc).__name__}: {exc}); pass "
                               "--trust-checkpoint to unpickle it without restrictions (runs code from the file)") from exc
        ckpt = torch.load(path, map_location="cpu", weights_only=False)
    sd = ckpt["state_dict"] if isinstance(ckpt, dict) and "state_dict" in ckpt else ckpt
    return {(k[len("model."):] if k.startswith("model.") else k): v for k, v in sd.items()}


def _attr(node):
    """yaml mapping -> AttrDict, recursively (what DiffusionQM9 reads its OmegaConf node through)."""
    from .diffusion import AttrDict
    if isinstance(node, dict):
        return AttrDict({k: _attr(v) for k, v in node.items()})
    if isinstance(node, list):
        return [_attr(v) for v in node]
    if isinstance(node, str):
        # PyYAML (YAML 1.1) reads `1e-4` as a string, OmegaConf - what the reference loads the file with - as a float
        import re
        if re.fullmatch(r"[-+]?(\d+\.?\d*|\.\d+)[eE][-+]?\d+", node):
            return float(node)
    return node


def load_model_config(path: str):
    """The reference's own model YAML (`endiffusion/conf/model/ddpmgblur.yaml`: `_target_` + a `cfg:` block, which Hydra hands
    to `DiffusionQM9.__init__` as `cfg`, sampler.py:20-22) -> the AttrDict this package's DiffusionQM9 takes.  `analyze` (the
    node-count histogram, `conf/analyze/GEOM.yaml`) is resolved the way a Hydra run does - relative to the directory that holds
    `conf/` - and falls back to the built-in copy of that histogram when the file is not there."""
    import yaml
    with open(path) as fh:
        doc = yaml.safe_load(fh)
    if not isinstance(doc, dict):
        raise ValueError(f"{path}: not a mapping")
    target = doc.get("_target_")
    if target is not None and not str(target).endswith("DiffusionQM9"):
        raise ValueError(f"{path}: _target_ {target!r} is not the coarse-grained diffusion model")
    cfg = _attr(doc.get("cfg", doc))
    for key in ("dynamics", "timesteps", "noise_schedule", "node_coarse_type"):
        if key not in cfg:
            raise ValueError(f"{path}: missing key {key!r} (expected the layout of conf/model/ddpmgblur.yaml)")
    an = cfg.get("analyze")
    if isinstance(an, str) and not os.path.isabs(an):
        here = os.path.dirname(os.path.abspath(path))
        tried = [os.path.join(base, an) for base in (os.path.dirname(os.path.dirname(here)), os.path.dirname(here), here, os.getcwd())]
        found = [p for p in tried if os.path.isfile(p)]
        cfg["analyze"] = found[0] if found else None
    return cfg


def load_sample_config(path: str) -> Tuple[int, int]:
    """`conf/sample/default.yaml` -> (batch_size, num_batches), the keyword arguments of `sample_batches` (sampler.py:38)."""
    import yaml
    with open(path) as fh:
        doc = yaml.safe_load(fh) or {}
    return int(doc["batch_size"]), int(doc["num_batches"])


def write_results(path: str, results: List[dict], test_names: Optional[list] = None) -> None:
    """The reference's output file: one pickle holding the tuple (results, test_names) (sampler.py:39-41)."""
    with open(path, "wb") as f:
        pickle.dump((results, [] if test_names is None else test_names), f)


def read_results(path: str) -> Tuple[List[dict], list]:
    with open(path, "rb") as f:
        res = pickle.load(f)
    return res[0], res[1]


def read_known(path: str) -> List[dict]:
    """`--known`: a list of {'x': [k,3], 'h': [k,8]} - `.pt` files through torch.load(weights_only=True), anything else as a pickle
    of the list or of the sampler's (results, test_names) tuple.  An entry may hold 'x' alone or 'h' alone (partial knowledge) and
    boolean 'x_mask' [k] / 'h_mask' [k] or [k,8] (`sample_grow`)."""
    if path.endswith(".pt"):
        obj = torch.load(path, map_location="cpu", weights_only=True)
    else:
        with open(path, "rb") as f:
            obj = pickle.load(f)
    if isinstance(obj, tuple) and len(obj) == 2 and isinstance(obj[0], list):
        obj = obj[0]
    if not isinstance(obj, list) or not all(isinstance(m, dict) and ("x" in m or "h" in m) for m in obj):
        raise ValueError(f"{path}: expected a list of {{'x', 'h'}} dicts (the sampler's output format; 'x' or 'h' alone: that part)")
    return obj


def known_parts(known: List[dict], parts: str) -> List[dict]:
    """`--known-parts`: every entry narrowed to its positions ("x") or its features ("h"); "both" hands them on as they are."""
    if parts == "both":
        return known
    drop = ("h", "h_mask") if parts == "x" else ("x", "x_mask")
    out = [{k: v for k, v in m.items() if k not in drop} for m in known]
    if not all(parts in m for m in out):
        raise ValueError(f"--known-parts {parts}: an entry of --known holds no '{parts}'")
    return out


def known_rows(m: dict) -> int:
    return int((m["x"] if m.get("x") is not None else m["h"]).shape[0])


class _DefaultEta(float):
    """The default of --eta, told apart from an explicit `--eta 1` by identity (--solver dpm2m defaults to eta = 0)."""


_ETA_DEFAULT = _DefaultEta(1.0)


def parse_args(argv=None):
    """The command line, checked: every argument error ends here (SystemExit), before a device is opened."""
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--checkpoint", default=None, help="reference Lightning checkpoint (.ckpt); random init if omitted")
    ap.add_argument("--batch-size", type=int, default=2)        # conf/sample/default.yaml:1
    ap.add_argument("--num-batches", type=int, default=16)      # conf/sample/default.yaml:2
    ap.add_argument("--out", default=None, help="output pickle (default: sample_results.pkl; with --score: scores.pkl)")
    ap.add_argument("--hidden-nf", type=int, default=256)
    ap.add_argument("--n-layers", type=int, default=6)
    ap.add_argument("--timesteps", type=int, default=1000)
    ap.add_argument("--context", type=float, nargs="*", default=None,
                    help="context values cycled over batches (needs a model with context_node_nf=1)")
    ap.add_argument("--precision", choices=["fp32", "fp16x3"], default="fp32",
                    help="fp32: exact fp32 matrix instructions (the reference's arithmetic); fp16x3: fp32-accurate two-way FP16 "
                         "split on the matrix cores, ~2.4x faster (recommended for sampling)")
    ap.add_argument("--trust-checkpoint", action="store_true",
                    help="allow the unrestricted unpickler for checkpoints that weights_only=True rejects")
    ap.add_argument("--seed", type=int, default=2022)
    ap.add_argument("--model-config", default=None,
                    help="the reference's model YAML (conf/model/ddpmgblur.yaml); overrides --hidden-nf / --n-layers / --timesteps")
    ap.add_argument("--sample-config", default=None,
                    help="the reference's sample YAML (conf/sample/default.yaml: batch_size, num_batches)")
    ap.add_argument("--known", default=None,
                    help="fragment growing: file with the fragments to keep (the sampler's output format); needs --grow")
    ap.add_argument("--grow", type=int, default=None, help="fragments to add to each molecule of --known")
    ap.add_argument("--known-parts", choices=["x", "h", "both"], default=None,
                    help="keep only that part of every entry of --known (default both): h = the fragments are known and their "
                         "positions are sampled (`--known lead.pkl --known-parts h --grow 0` lays a lead's fragments out again), x = the "
                         "positions are known and the fragments are sampled (`--known-parts x --grow 0` re-assigns fragments to a "
                         "lead's positions); combines with everything --known / --grow combines with.  With --restraint-frame known "
                         "and --known-parts h there is no frame: the tables are read in the model's frame (tau = 0).  Mechanism "
                         "only: how well the sampled part fits the known one is for you to validate")
    ap.add_argument("--resamplings", type=int, default=1,
                    help="network calls per diffusion step of --known runs (1: plain replacement; more: RePaint-style resampling)")
    ap.add_argument("--steps", type=int, default=None,
                    help="few-step sampling: K <= timesteps transitions on a sub-sequence of the trained grid (default: all of "
                         "them); combinable with --known/--grow.  Mechanism only: which K keeps sample quality is for you to validate")
    ap.add_argument("--eta", type=float, default=_ETA_DEFAULT,
                    help="1: ancestral steps (default); 0 <= eta < 1: DDIM-family update, 0 = noise-free (not with --known)")
    ap.add_argument("--spacing", choices=["uniform", "quadratic"], default="uniform", help="how --steps spreads over the grid")
    ap.add_argument("--solver", choices=["ddim", "dpm2m", "sde2m"], default=None,
                    help="dpm2m: second-order multistep sampling (DPM-Solver++ 2M) on the --steps path, deterministic (eta = 0) at no "
                         "extra network call; combines with --steps / --spacing, --guidance and --vary, not with --known / --grow or "
                         "--eta other than 0.  sde2m: its stochastic counterpart (SDE-DPM-Solver++ 2M): second order with the ancestral "
                         "noise on the path (eta = 1), so it also combines with --restraints and --particles; not with --known / "
                         "--grow, --score, --interpolate or --eta other than 1.  Mechanism only: which K keeps sample quality is for you "
                         "to validate")
    ap.add_argument("--no-lower-order-final", dest="lower_order_final", action="store_false",
                    help="with --solver dpm2m / sde2m: keep the second-order correction on the last transition too")
    ap.add_argument("--score", default=None, metavar="FILE",
                    help="score the molecules of FILE (a sample_results.pkl or a bare list in the sampler's output format) instead of "
                         "sampling: the variational bound with every timestep evaluated, one value per molecule, written to --out.  "
                         "Mechanism only: scores of untrained weights mean nothing chemically")
    ap.add_argument("--terms", type=int, default=None,
                    help="with --score: evaluate K <= timesteps uniformly spaced terms of the bound (default: all of them)")
    ap.add_argument("--vary", default=None, metavar="FILE",
                    help="variations of the molecules of FILE (the sampler's output format): noise each to --t-start and run the "
                         "reverse chain from there; combines with --steps / --eta / --spacing.  Mechanism only")
    ap.add_argument("--t-start", type=int, default=None,
                    help="with --vary: the grid index in 1 .. timesteps the molecules are noised to (how far variations drift)")
    ap.add_argument("--variants", type=int, default=1, help="with --vary: results per input molecule")
    ap.add_argument("--interpolate", default=None, metavar="FILE",
                    help="interpolate between consecutive molecules of FILE: encode (eta = 0 upwards), slerp, decode --frames "
                         "molecules per pair; pairs of unequal size are skipped.  Mechanism only")
    ap.add_argument("--frames", type=int, default=None, help="with --interpolate: molecules per pair, both ends included (>= 2)")
    ap.add_argument("--guidance", type=float, default=None, metavar="W",
                    help="classifier-free guidance scale (needs --context): every network call runs under the context and under "
                         "the null context, eps_u + W (eps_c - eps_u) goes into the update; combines with --steps / --eta / "
                         "--spacing, --known / --grow and --vary.  Mechanism only: the checkpoint must have been trained with "
                         "context dropout, and which W helps is for you to validate")
    ap.add_argument("--guidance-rescale", type=float, default=0.0, metavar="PHI",
                    help="with --guidance: rescale the combination towards the spread of the conditional prediction (0 .. 1)")
    ap.add_argument("--null-context", type=float, nargs="+", default=None, metavar="V",
                    help="with --guidance: the null context (one value, or one per context column; default 0)")
    ap.add_argument("--chain", type=int, default=None, metavar="FRAMES",
                    help="record the trajectory (the reference's sample_chain): every molecule also gets 'chain_x' / 'chain_h' "
                         "[FRAMES, n, .] and 'chain_t' [FRAMES] - FRAMES <= the number of transitions, frame 0 the result itself; "
                         "combines with everything --steps combines with (--eta / --spacing / --solver, --guidance, --known / "
                         "--grow, --vary), not with --score / --interpolate")
    ap.add_argument("--record", choices=["z", "x0"], default=None,
                    help="with --chain: keep the states (z, default) or the network's data prediction of the same transitions (x0)")
    ap.add_argument("--restraints", default=None, metavar="FILE.json",
                    help="restraint-guided sampling: a JSON object with the keys obstacles [[y_x, y_y, y_z, r, k]], pairs [[i, j, lo, "
                         "hi, k]], anchors [[i, a_x, a_y, a_z, r, k]] shared by all molecules, in data units in the MODEL'S frame (the "
                         "molecule's centre of mass is the origin); the gradient of the energy on the network's data prediction goes "
                         "into every transition.  The key features {bands: {lo, hi, k} | {target, tol, k}, sums: [{coef, lo, hi, k, "
                         "reduce}]} restrains the feature channels h: bands on single elements, windows on molecule-wide sums or "
                         "means.  Combines with everything --steps combines with (--eta / --spacing / --solver, "
                         "--guidance, --chain, --vary) except --known / --grow.  Mechanism only: which scale, schedule and clip help "
                         "is for you to validate")
    ap.add_argument("--restraint-frame", choices=["model", "known"], default=None,
                    help="with --restraints: the frame the tables are in - the model's (default: the molecule's centre of mass at the "
                         "origin) or, with --known / --grow only, the coordinates of the known fragments as given in FILE (a pocket's, "
                         "for instance: grow without clashing with protein atoms); known makes --restraints legal with --known / --grow")
    ap.add_argument("--restraint-scale", type=float, default=None, metavar="S", help="with --restraints: the scale (default 1)")
    ap.add_argument("--restraint-schedule", choices=["score", "sigma"], default=None,
                    help="with --restraints: the weight of transition k, nv0 sigma_t / alpha_t (score, default) or sigma_t")
    ap.add_argument("--restraint-clip", type=float, default=None, metavar="C",
                    help="with --restraints: the largest step per node in noise-prediction units (default: none)")
    ap.add_argument("--particles", type=int, default=None, metavar="P",
                    help="with --restraints and --steer-scale: steered sampling - every P consecutive molecules of a batch are the "
                         "particles of one group (one drawn size, equal context), weighted at every transition by the change of "
                         "their restraint energy and resampled inside the device loop when their effective sample size falls below "
                         "--steer-ess * P; --batch-size (and --variants) must be multiples of P.  Without --restraint-scale the "
                         "gradient update is off (selection only).  Results also hold steer_logw / steer_root / steer_group.  "
                         "Mechanism only: which P, scale and threshold help is for you to validate")
    ap.add_argument("--steer-scale", type=float, default=None, metavar="S", help="with --particles: beta, the weight of the energy "
                    "change in the log-weights")
    ap.add_argument("--steer-ess", type=float, default=None, metavar="R", help="with --particles: resample below R * P (default 0.5)")
    ap.add_argument("--diverse", type=int, default=None, metavar="P",
                    help="with --diverse-length: diverse sampling - every P consecutive molecules of a batch (with --vary: the variants "
                         "of one input) form a group (one drawn size, equal context) whose members repel each other at every "
                         "transition by the aligned RMSD of their data predictions, inside the device loop; --batch-size (and "
                         "--variants) must be multiples of P (at most 32).  A gradient, not a selection: it combines with everything "
                         "--steps combines with, --eta 0 and --solver dpm2m included, except --known / --grow and --particles.  "
                         "Results also hold diversity_group / diversity_rmsd.  Mechanism only: which length and strength help is "
                         "for you to validate")
    ap.add_argument("--diverse-length", type=float, default=None, metavar="L", help="with --diverse: the width of the Gaussian in the "
                    "units of the aligned RMSD")
    ap.add_argument("--diverse-strength", type=float, default=None, metavar="S", help="with --diverse: kappa (default 1)")
    ap.add_argument("--diverse-clip", type=float, default=None, metavar="C",
                    help="with --diverse: the largest step per node in noise-prediction units (default: none)")
    ap.add_argument("--diverse-schedule", choices=["score", "sigma"], default=None,
                    help="with --diverse: the weight of transition k, nv0 sigma_t / alpha_t (score, default) or sigma_t")
    ap.add_argument("--correctors", type=int, default=None, metavar="C",
                    help="predictor-corrector sampling: C (1 .. 8) Langevin steps at the departure level of every transition, on the "
                         "score the network and the call's terms define (k_langevin_step); each costs one more network call.  Combines "
                         "with everything --steps combines with except --known / --grow and --particles.  Mechanism only: r = 0.16 is "
                         "Song et al.'s image value; which C and r help is for a trained checkpoint to show.")
    ap.add_argument("--corrector-snr", type=float, default=None, metavar="R", help="with --correctors: Song's signal-to-noise ratio r of "
                    "mode snr (default 0.16)")
    ap.add_argument("--corrector-mode", choices=["snr", "fixed"], default=None,
                    help="with --correctors: the gain follows the norms of noise and score per molecule (snr, default), or is "
                         "--corrector-gain (fixed)")
    ap.add_argument("--corrector-gain", type=float, default=None, metavar="G", help="with --correctors --corrector-mode fixed: the gain g")
    args = ap.parse_args(argv)
    if args.correctors is None and (args.corrector_snr is not None or args.corrector_mode is not None or args.corrector_gain is not None):
        ap.error("--corrector-snr / --corrector-mode / --corrector-gain need --correctors")
    if args.correctors is not None:
        if not 1 <= args.correctors <= 8:
            ap.error("--correctors must lie in 1 .. 8")
        if (args.corrector_mode == "fixed") != (args.corrector_gain is not None):
            ap.error("--corrector-gain and --corrector-mode fixed go together")
        if args.corrector_mode == "fixed" and args.corrector_snr is not None:
            ap.error("--corrector-snr goes with --corrector-mode snr")
        for name, v in (("--corrector-snr", args.corrector_snr), ("--corrector-gain", args.corrector_gain)):
            if v is not None and not (math.isfinite(v) and v >= 0.0):
                ap.error(f"{name} must be finite and >= 0")
        if args.particles is not None:
            ap.error("--correctors does not combine with --particles (the particles' weights follow the predictor's moves alone)")
        if args.known is not None or args.grow is not None:
            ap.error("--correctors does not combine with --known / --grow (the replacement would have to be redone behind every corrector step)")
        if args.score is not None or args.interpolate is not None:
            ap.error("--correctors does not combine with --score / --interpolate")
    if (args.diverse is None) != (args.diverse_length is None):
        ap.error("--diverse and --diverse-length go together")
    if args.diverse is None and (args.diverse_strength is not None or args.diverse_clip is not None or args.diverse_schedule is not None):
        ap.error("--diverse-strength / --diverse-clip / --diverse-schedule need --diverse and --diverse-length")
    if args.diverse is not None:
        if not 1 <= args.diverse <= 32:
            ap.error("--diverse must lie in 1 .. 32")
        if not (math.isfinite(args.diverse_length) and args.diverse_length > 0.0):
            ap.error("--diverse-length must be finite and > 0")
        if args.diverse_strength is not None and not (math.isfinite(args.diverse_strength) and args.diverse_strength >= 0.0):
            ap.error("--diverse-strength must be finite and >= 0")
        if args.diverse_clip is not None and not args.diverse_clip > 0.0:
            ap.error("--diverse-clip must be > 0")
        if args.particles is not None:
            ap.error("--diverse does not combine with --particles (both lay groups over the batch)")
        if args.known is not None or args.grow is not None:
            ap.error("--diverse does not combine with --known / --grow (inpainting re-centres on the known fragments)")
        if args.score is not None or args.interpolate is not None:
            ap.error("--diverse does not combine with --score / --interpolate")
        if args.batch_size % args.diverse or (args.vary is not None and args.variants % args.diverse):
            ap.error("--batch-size (and with --vary, --variants) must be a multiple of --diverse")
    if (args.particles is None) != (args.steer_scale is None):
        ap.error("--particles and --steer-scale go together")
    if args.steer_ess is not None and args.particles is None:
        ap.error("--steer-ess needs --particles and --steer-scale")
    if args.particles is not None:
        if args.restraints is None:
            ap.error("--particles needs --restraints (the particles are weighted by their restraint energy)")
        if not 1 <= args.particles <= 256:
            ap.error("--particles must lie in 1 .. 256")
        if not (math.isfinite(args.steer_scale) and args.steer_scale >= 0.0):
            ap.error("--steer-scale must be finite and >= 0")
        if args.steer_ess is not None and not 0.0 < args.steer_ess <= 1.0:
            ap.error("--steer-ess must lie in (0, 1]")
        if args.batch_size % args.particles or (args.vary is not None and args.variants % args.particles):
            ap.error("--batch-size (and with --vary, --variants) must be a multiple of --particles")
    if args.restraints is None and (args.restraint_scale is not None or args.restraint_schedule is not None
                                    or args.restraint_clip is not None or args.restraint_frame is not None):
        ap.error("--restraint-scale / --restraint-schedule / --restraint-clip / --restraint-frame need --restraints")
    if args.restraints is not None:
        if args.restraint_frame == "known":
            if args.known is None or args.grow is None:
                ap.error("--restraint-frame known needs --known / --grow (the frame of the known fragments)")
            if args.particles is not None:
                ap.error("--restraint-frame known does not combine with --particles (inpainting is not steered)")
        elif args.known is not None or args.grow is not None:
            ap.error("--restraints does not combine with --known / --grow (inpainting re-centres on the known fragments; "
                     "--restraint-frame known reads the tables in the fragments' own coordinates)")
        if args.score is not None or args.interpolate is not None:
            ap.error("--restraints does not combine with --score / --interpolate")
        if args.restraint_clip is not None and not args.restraint_clip > 0.0:
            ap.error("--restraint-clip must be > 0")
        if args.restraint_scale is not None and not math.isfinite(args.restraint_scale):
            ap.error("--restraint-scale must be finite")
        if args.restraint_scale is None and args.particles is None:
            args.restraint_scale = 1.0
    if args.record is not None and args.chain is None:
        ap.error("--record needs --chain")
    if args.chain is not None and args.chain < 1:
        ap.error("--chain must be >= 1")
    if args.chain is not None and (args.score is not None or args.interpolate is not None):
        ap.error("--chain does not combine with --score / --interpolate")
    if args.guidance is not None and not args.context:
        ap.error("--guidance needs --context")
    if args.guidance is None and (args.guidance_rescale != 0.0 or args.null_context is not None):
        ap.error("--guidance-rescale and --null-context need --guidance")
    if not (0.0 <= args.guidance_rescale <= 1.0):
        ap.error("--guidance-rescale must be in [0, 1]")
    if args.guidance is not None and (args.score is not None or args.interpolate is not None):
        ap.error("--guidance does not combine with --score / --interpolate")
    modes = [n for n in ("score", "known", "vary", "interpolate") if getattr(args, n) is not None]
    if len(modes) > 1:
        ap.error("--" + " and --".join(modes) + " do not combine")
    if (args.vary is None) != (args.t_start is None):
        ap.error("--vary and --t-start go together")
    if args.vary is not None and (args.t_start < 1 or args.variants < 1):
        ap.error("--t-start and --variants must be >= 1")
    if args.variants != 1 and args.vary is None:
        ap.error("--variants needs --vary")
    if (args.interpolate is None) != (args.frames is None):
        ap.error("--interpolate and --frames go together")
    if args.interpolate is not None and args.frames < 2:
        ap.error("--frames must be >= 2")
    if args.interpolate is not None and args.eta != 1.0:
        ap.error("--eta does not combine with --interpolate (frames are decoded with eta = 0)")
    if args.score is not None and (args.known is not None or args.grow is not None or args.steps is not None):
        ap.error("--score does not combine with --known / --grow / --steps (it samples nothing)")
    if args.terms is not None and args.score is None:
        ap.error("--terms needs --score")
    if args.terms is not None and args.terms < 1:
        ap.error("--terms must be >= 1")
    if args.out is None:
        args.out = "scores.pkl" if args.score is not None else "sample_results.pkl"
    if args.steps is not None and args.steps < 1:
        ap.error("--steps must be >= 1")
    if not args.lower_order_final and args.solver not in ("dpm2m", "sde2m"):
        ap.error("--no-lower-order-final needs --solver dpm2m or sde2m")
    if args.solver == "sde2m":
        if args.known is not None or args.grow is not None:
            ap.error("--solver sde2m does not combine with --known / --grow (inpainting takes ancestral steps)")
        if args.score is not None or args.interpolate is not None:
            ap.error("--solver sde2m does not combine with --score / --interpolate")
        if args.eta is not _ETA_DEFAULT and args.eta != 1.0:
            ap.error("--solver sde2m draws the ancestral noise: --eta must be 1 (or left out)")
        args.eta = 1.0
    if args.solver == "dpm2m":
        if args.known is not None or args.grow is not None:
            ap.error("--solver dpm2m does not combine with --known / --grow (inpainting takes ancestral steps)")
        if args.score is not None or args.interpolate is not None:
            ap.error("--solver dpm2m does not combine with --score / --interpolate")
        if args.eta is not _ETA_DEFAULT and args.eta != 0.0:
            ap.error("--solver dpm2m is deterministic: --eta must be 0 (or left out)")
        args.eta = 0.0
    args.eta = float(args.eta)
    if not (0.0 <= args.eta <= 1.0):
        ap.error("--eta must be in [0, 1]")
    if args.known is not None and args.eta < 1.0:
        ap.error("--eta < 1 does not combine with --known (inpainting takes ancestral steps)")
    if (args.known is None) != (args.grow is None):
        ap.error("--known and --grow go together")
    if args.known_parts is not None and args.known is None:
        ap.error("--known-parts needs --known")
    if args.known is not None and (args.grow < 0 or args.resamplings < 1):
        ap.error("--grow must be >= 0 and --resamplings >= 1")
    if args.sample_config:
        args.batch_size, args.num_batches = load_sample_config(args.sample_config)
    return args


def main(argv=None) -> int:
    args = parse_args(argv)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    dev = torch.device("cuda", local_rank)
    torch.cuda.set_device(dev)
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)

    ctx_nf = 1 if args.context else 0
    if args.model_config:
        cfg = load_model_config(args.model_config)
        if ctx_nf:
            cfg.dynamics.context_node_nf = ctx_nf
        model = DiffusionQM9(cfg)
    else:
        model = DiffusionQM9(default_config(hidden_nf=args.hidden_nf, n_layers=args.n_layers, context_node_nf=ctx_nf,
                                            timesteps=args.timesteps))
    if rank == 0 and args.checkpoint:
        model.load_state_dict(load_reference_state_dict(args.checkpoint, args.trust_checkpoint))
    model = model.to(dev)
    model.dynamics.precision = args.precision
    model.seed = args.seed
    if args.steps is not None and args.steps > model.T:
        raise SystemExit(f"--steps {args.steps} exceeds the model's {model.T} timesteps")
    model.sample_steps, model.sample_eta, model.sample_spacing = args.steps, args.eta, args.spacing
    if args.solver in ("dpm2m", "sde2m"):
        model.sample_solver, model.sample_lower_order_final = args.solver, args.lower_order_final
    if args.guidance is not None:
        model.guidance_scale, model.guidance_rescale = args.guidance, args.guidance_rescale
        if args.null_context is not None:
            model.null_context = args.null_context[0] if len(args.null_context) == 1 else list(args.null_context)
    if world > 1:
        broadcast_model_weights(model, src=0)
    chain = {} if args.chain is None else {"keep_frames": args.chain, "record": args.record}
    if args.restraints is not None:
        from .restraints import Restraints
        chain.update(restraints=Restraints.from_json(args.restraints), restraint_scale=args.restraint_scale,
                     restraint_schedule=args.restraint_schedule, restraint_clip=args.restraint_clip)
        if args.restraint_frame is not None:
            chain.update(restraint_frame=args.restraint_frame)
    if args.particles is not None:
        chain.update(particles=args.particles, steer_scale=args.steer_scale, steer_ess=args.steer_ess)
    if args.diverse is not None:
        from .diversity import Diversity
        chain.update(diversity=Diversity(args.diverse, args.diverse_length, 1.0 if args.diverse_strength is None else args.diverse_strength,
                                         schedule=args.diverse_schedule or "score", clip=args.diverse_clip))
    if args.correctors is not None:
        from .corrector import Corrector
        if args.corrector_mode == "fixed":
            chain.update(corrector=Corrector(args.correctors, mode="fixed", gain=args.corrector_gain))
        else:
            chain.update(corrector=Corrector(args.correctors, snr=0.16 if args.corrector_snr is None else args.corrector_snr))

    if args.score is not None:
        if world > 1:
            raise SystemExit("--score runs in a single process")
        if args.terms is not None and args.terms > model.T:
            raise SystemExit(f"--terms {args.terms} exceeds the model's {model.T} timesteps")
        scores = model.score(read_known(args.score), dev, batch_size=max(1, args.batch_size), terms=args.terms)
        with open(args.out, "wb") as f:
            pickle.dump(scores, f)
        return 0

    if args.vary is not None:
        if world > 1:
            raise SystemExit("--vary runs in a single process")
        if args.t_start > model.T:
            raise SystemExit(f"--t-start {args.t_start} exceeds the model's {model.T} timesteps")
        if args.steps is not None and args.steps > args.t_start:
            raise SystemExit(f"--steps {args.steps} exceeds the {args.t_start} steps below --t-start")
        model.sample_steps = None               # --steps spreads over the t_start steps below the start, not over the whole grid
        write_results(args.out, model.vary(read_known(args.vary), dev, args.t_start, n_variants=args.variants,
                                           batch_size=max(1, args.batch_size), steps=args.steps, **chain))
        return 0

    if args.interpolate is not None:
        if world > 1:
            raise SystemExit("--interpolate runs in a single process")
        model.sample_steps = None
        mols = read_known(args.interpolate)
        frames: List[dict] = []
        for i, (a, b) in enumerate(zip(mols[:-1], mols[1:])):
            if int(a["x"].shape[0]) != int(b["x"].shape[0]):
                print(f"--interpolate: skipping pair {i}, {i + 1}: {int(a['x'].shape[0])} and {int(b['x'].shape[0])} nodes")
                continue
            frames.extend(model.interpolate(a, b, args.frames, dev, steps=args.steps))
        write_results(args.out, frames)
        return 0

    if args.known is not None:
        if world > 1:
            raise SystemExit("--known runs in a single process")
        known = known_parts(read_known(args.known), args.known_parts or "both")
        grown: List[dict] = []
        for b, lo in enumerate(range(0, len(known), max(1, args.batch_size))):
            part = known[lo:lo + max(1, args.batch_size)]
            ctx = None if not args.context else args.context[b % len(args.context)]
            grown.extend(model.sample_grow(part, [known_rows(m) + args.grow for m in part], dev, context=ctx,
                                           resamplings=args.resamplings, sample_id_base=lo, **chain))
        write_results(args.out, grown)
        return 0

    steered = args.particles is not None and args.particles > 1 and args.steer_scale != 0.0
    group = args.particles if steered else chain["diversity"].P if "diversity" in chain and chain["diversity"].active else 1
    torch.manual_seed(args.seed)           # the node-count draw uses torch's CPU generator (distributions.py)
    results: List[dict] = []
    first, count = shard_sample_ids(0, args.num_batches, rank, world)      # whole batches per rank
    for b in range(args.num_batches):
        if not (first <= b < first + count):
            # advance the node-count generator over batches owned by other ranks, so the global sequence of
            # molecule sizes (and, with the counter-based noise, every sample) is independent of the world size
            model.nodes_dist.sample(args.batch_size // group)    # (a steered or diverse batch draws one size per group)
            continue
        ctx = None if not args.context else args.context[b % len(args.context)]
        results.extend(model.sample(args.batch_size, dev, context=ctx, sample_id_base=b * args.batch_size, **chain))
    if world == 1:
        write_results(args.out, results)
        return 0
    write_results(f"{args.out}.rank{rank}", results)
    import torch.distributed as dist
    dist.barrier()
    if rank == 0:
        merged: List[dict] = []
        for r in range(world):
            merged.extend(read_results(f"{args.out}.rank{r}")[0])
            os.remove(f"{args.out}.rank{r}")
        write_results(args.out, merged)
    dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
