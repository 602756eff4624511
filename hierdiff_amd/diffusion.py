"""The reference's `DiffusionQM9` (endiffusion/train_module/diffusion_qm9.py) on MI355X: sampling, loss / NLL, training hooks.

Same entry points and result format as the reference:
  DiffusionQM9.sample(num_samples, device, context=None, pocket_cond=None)        :347-395
  DiffusionQM9.sample_batches(batch_size, num_batches, device, context_range, ..) :397-436
  DiffusionQM9.sample_p_zs_given_zt / sample_p_xh_given_z0 / phi / sigma / alpha   :135-158, 294-345
plus the EDM-style signature named by the north star,
  EnVariationalDiffusion.sample(n_samples, n_nodes, node_mask, edge_mask, context, fix_noise=False)
  (endiffusion/equivariant_diffusion/en_diffusion.py:634-667; dead code in the reference).

Every reverse chain runs inside libhierdiff_hip.so: the plain 1000-step loop (hd_sample_loop; inpainting: hd_sample_loop_inpaint)
or, for few-step, multistep, guided, restrained and recorded calls, the loop over a path of grid points (hd_sample_path,
hd_sample_path_inpaint, hd_sample_path_guided) - about 45 kernels per step at the headline batch, no host sync,
by default replayed from one captured hipGraph that is cached per topology.  Every sampling entry point is the same four steps:
the keywords resolved on the host (`plan.plan`), the device state (`_device_state`), the transitions (`_run`, the one place that
picks among the five loops) and the decode (`_decode`).  The loss / NLL value of the training half is available too (compute_loss,
nll, forward).
"""
from __future__ import annotations

import contextlib
import ctypes as C
import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from . import corrector as corrector_mod, diversity as diversity_mod, restraints as restraints_mod, steering as steering_mod
from .distributions import DistributionNodes
from .dynamics import EGNN_dynamics_QM9, Topology, _ptr, _stream
from .geom_stats import GEOM_FRAGMENT_HISTOGRAM
from .noise_model import (GammaNetwork, PredefinedNoiseSchedule, decode_coefficients, evaluate_gamma,
                          schedule_tables, sigma_and_alpha_t_given_s, step_coefficients)
from .plan import KEYWORDS, full_path, given, latent_path, plan as make_plan, unsupported

try:  # the reference class is a LightningModule; use it when the package exists so the module nests
    import pytorch_lightning as _pl  # type: ignore
    _Base = _pl.LightningModule
except Exception:  # pragma: no cover - not installed in this image
    _Base = nn.Module


class AttrDict(dict):
    """dict with attribute access, standing in for the OmegaConf node the reference passes around."""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e

    def __setattr__(self, k, v):
        self[k] = v


def default_config(hidden_nf: int = 256, n_layers: int = 6, context_node_nf: int = 0, timesteps: int = 1000,
                   inv_sublayers: int = 2, normalization_factor: float = 10.0) -> AttrDict:
    """The production hyper-parameters of endiffusion/conf/model/ddpmgblur.yaml:2-38."""
    return AttrDict(
        pocket=False, node_coarse_type="prop", loss_type="vlb", hcontinous=True, noise_schedule="learned",
        timesteps=timesteps, norm_values=[1.0, 1.0, 1.0], norm_biases=[None, 0.0, 0.0], parametrization="eps",
        include_charges=True, dataset="qm9", conditioning=[], data_augmentation=False,
        pre_noise=AttrDict(noise_schedule="learned", timesteps=timesteps, precision=1e-4),
        dynamics=AttrDict(in_node_nf=0, context_node_nf=context_node_nf, n_dims=3, hidden_nf=hidden_nf,
                          act_fn="silu", n_layers=n_layers, attention=True, condition_time=True, tanh=True,
                          mode="egnn_dynamics", norm_constant=0, inv_sublayers=inv_sublayers, sin_embedding=False,
                          normalization_factor=normalization_factor, aggregation_method="sum"),
        analyze=None,
    )


def _get(cfg, key, default=None):
    try:
        return cfg[key]
    except Exception:
        return getattr(cfg, key, default)


RESIDUE_LIST = ["ALA", "ARG", "ASN", "ASP", "CYS", "GLN", "GLU", "GLY", "HIS", "ILE", "LEU", "LYS", "MET", "PHE", "PRO",
                "SER", "THR", "TRP", "TYR", "VAL"]


def pocket_tensors(protein_data_all):
    """Padded pocket tensors [feat (long, 0 = pad), pos, node_mask, edge_mask] as `sample_batches` builds them
    (diffusion_qm9.py:399-420): residue type index + 1, all-pairs-minus-diagonal edge mask per pocket."""
    feats = [torch.tensor([RESIDUE_LIST.index(r) + 1 for r in p["residue_type"]]) for p in protein_data_all]
    poss = [torch.tensor(np.array(p["coord"])) for p in protein_data_all]
    n, pmax = len(feats), max(f.shape[0] for f in feats)
    feat = torch.zeros(n, pmax, dtype=torch.long)
    pos = torch.zeros(n, pmax, 3)
    nmask = torch.zeros(n, pmax, 1, dtype=torch.bool)
    emask = torch.zeros(n, pmax, pmax, dtype=torch.bool)
    for i, (f, p) in enumerate(zip(feats, poss)):
        k = f.shape[0]
        feat[i, :k] = f
        pos[i, :k] = p
        nmask[i, :k, 0] = True
        emask[i, :k, :k] = ~torch.eye(k, dtype=torch.bool)
    return [feat, pos, nmask, emask]


class DiffusionQM9(_Base):
    """Sampler with the reference's constructor contract: `DiffusionQM9(cfg)` where `cfg` carries the
    keys of conf/model/ddpmgblur.yaml (diffusion_qm9.py:37-115)."""

    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        self.pocket = bool(_get(cfg, "pocket", False))
        self.node_coarse_type = _get(cfg, "node_coarse_type")
        if self.node_coarse_type == "prop":
            self.in_node_nf = 8
        elif self.node_coarse_type == "elem":
            self.in_node_nf = 3
        else:
            raise NotImplementedError("node_coarse_type should be prop or elem")
        if self.pocket:
            self.pocket_embed = nn.Embedding(21, self.in_node_nf)       # diffusion_qm9.py:55-56
        dyn = dict(_get(cfg, "dynamics"))
        dyn["in_node_nf"] = self.in_node_nf
        assert _get(cfg, "loss_type") in {'vlb', 'l2'}
        self.loss_type = _get(cfg, "loss_type")
        self.include_charges = _get(cfg, "include_charges")
        assert _get(cfg, "parametrization") == 'eps'
        if _get(cfg, "noise_schedule") == 'learned':
            assert self.loss_type == 'vlb', 'A noise schedule can only be learned with a vlb objective.'
            self.gamma = GammaNetwork()
        else:
            self.gamma = PredefinedNoiseSchedule(**dict(_get(cfg, "pre_noise")))
        self.hcontinous = _get(cfg, "hcontinous")
        if dyn.get("condition_time", True):
            dyn["in_node_nf"] += 1
        self.dynamics = EGNN_dynamics_QM9(**dyn)
        self.n_dims = dyn["n_dims"]
        self.T = int(_get(cfg, "timesteps"))
        self.parametrization = _get(cfg, "parametrization")
        self.norm_values = list(_get(cfg, "norm_values"))
        self.norm_biases = list(_get(cfg, "norm_biases"))
        # data scaling (diffusion_qm9.py:103-104, 165-179; production: [1,1,1] / [None,0,0], ddpmgblur.yaml:10-11).  The library's
        # decode kernel returns normalised x / h; `_final_decode` applies `unnormalize` when the values are not the unit ones.
        self._unit_norm = [float(v) for v in self.norm_values] == [1.0, 1.0, 1.0] and \
            all(float(b or 0.0) == 0.0 for b in self.norm_biases)
        self.register_buffer('buffer', torch.zeros(1))
        if _get(cfg, "noise_schedule") != 'learned':
            self.check_issues_norm_values()
        self.data_augmentation = _get(cfg, "data_augmentation", False)
        analyze = _get(cfg, "analyze", None)
        if isinstance(analyze, dict):
            histogram = analyze
        elif isinstance(analyze, str):
            import yaml
            with open(analyze) as fh:
                histogram = yaml.safe_load(fh)
        else:
            histogram = GEOM_FRAGMENT_HISTOGRAM
        self.nodes_dist = DistributionNodes(histogram=histogram)
        # sampling knobs of this implementation (not in the reference)
        self.noise_mode = "philox"      # "philox": in-kernel counter RNG; "torch": torch.randn draws
        self.seed = 2022
        self.use_graph = True
        # sample_batches: molecules of consecutive batches run as ONE device batch of at most `merge_batches` molecules and
        # `merge_edges` directed edges (merge_batches = 0: one device batch per call of the reference's loop).  Samples are
        # bit-identical either way (a sample depends on its global id only).  900,000 edges are four headline batches
        # (256 x 30 x 29 each): measured on 8 x 256 GEOM-sized molecules (scratch/geom_job_time.py, fp32) the loop runs at
        # 120.5 molecules/s, device batches of 225 k / 450 k / 900 k edges at 142.5 / 148.8 / 159.2.
        self.merge_batches = 4096
        self.merge_edges = 900_000
        self.debug_checks = False       # True re-enables the reference's host-synchronising asserts
        #: training-mode loss around the network call as two fused launches per direction (csrc/k_loss.hpp) instead of ~350 torch
        #: launches; False = the torch-op path (same arithmetic; what evaluation, pocket models and the CPU run)
        self.fused_loss = True
        self.schedule_gammas = None     # optional [T+1] gamma grid overriding the network (replay a run)
        # "fp64" (default): the schedule network is evaluated once in float64 on the host and rounded - the same table on
        # every machine.  "fp32": evaluated like the reference (float32, a [B,1] column per grid value, CPU BLAS): agrees
        # run for run with a CPU reference on the same host, host-dependent otherwise.
        self.schedule_eval = "fp64"
        self._sched_key = None
        self._sched = None
        # few-step sampling (hierdiff_amd/paths.py): defaults of the `steps` / `eta` / `spacing` / `timesteps` keywords of the
        # sampling entry points.  None / 1.0 = the full chain through the plain loop, i.e. nothing changes.
        self.sample_steps = None
        self.sample_eta = 1.0
        self.sample_spacing = "uniform"
        self.sample_timesteps = None
        # default of the `solver` keyword: None / "ddim" = the first-order updates above; "dpm2m" = DPM-Solver++(2M), eta = 0;
        # "sde2m" = SDE-DPM-Solver++(2M), second order with the ancestral noise (eta = 1)
        self.sample_solver = None
        self.sample_lower_order_final = True
        self._force_path_loop = False   # tests: run the identity path (K = T, eta = 1) through the path loop instead of the plain one
        # classifier-free guidance (hierdiff_amd/guidance.py): defaults of the `guidance_scale` / `guidance_context` /
        # `guidance_rescale` keywords of the sampling entry points.  None = unguided, i.e. nothing changes.  `null_context`: a float
        # or a [C] vector, the context a molecule is given in place of its own - by guided sampling (the second network call) and by
        # context dropout in training (`context_drop_prob`, one draw per molecule; `context_drop_generator`: optional CPU generator)
        self.guidance_scale = None
        self.guidance_context = None
        self.guidance_rescale = 0.0
        self.null_context = _get(cfg, "null_context", 0.0) or 0.0
        self.context_drop_prob = float(_get(cfg, "context_drop_prob", 0.0) or 0.0)
        self.context_drop_generator = None
        # restraint-guided sampling (hierdiff_amd/restraints.py): defaults of the `restraints` / `restraint_scale` / `restraint_schedule`
        # / `restraint_clip` keywords of the sampling entry points.  No restraints, or a scale of None / 0 = nothing changes.
        self.restraints = None
        self.restraint_scale = None
        self.restraint_schedule = "score"
        self.restraint_clip = None
        # the frame the tables are read in: None / "model" (the model's, everywhere) or "known" (the known fragments' of
        # sample_inpaint / sample_grow / inpaint_steps, which take restraints only then)
        self.restraint_frame = None
        # steered sampling (hierdiff_amd/steering.py): defaults of the `particles` / `steer_scale` / `steer_ess` keywords.  particles of
        # None or 1, or a steer_scale of None or 0 = nothing changes.  `steer_last`: the `steering.Result` of the last steered call.
        self.particles = None
        self.steer_scale = None
        self.steer_ess = None
        self.steer_last = None
        # diverse sampling (hierdiff_amd/diversity.py): the default of the `diversity` keyword (a `diversity.Diversity`; None, particles
        # = 1, or a strength or scale of 0 = nothing changes).  `diversity_last`: the `diversity.Result` of the last diverse call.
        self.diversity = None
        self.diversity_last = None
        # predictor-corrector sampling (hierdiff_amd/corrector.py): the default of the `corrector` keyword (a `corrector.Corrector`; None,
        # steps = 0 or a strength of 0 = nothing changes).  `corrector_last`: [C, B] float64, the gains of the last transition of the last
        # corrected call (0 where a molecule kept its bits).
        self.corrector = None
        self.corrector_last = None

    def check_issues_norm_values(self, num_stdevs=8):
        """diffusion_qm9.py:117-131 (predefined schedules only)."""
        sigma_0 = float(torch.sqrt(torch.sigmoid(self.gamma(torch.zeros((1, 1))))).reshape(-1)[0])
        max_norm_value = max(self.norm_values[1], self.norm_values[2])
        if sigma_0 * num_stdevs > 1. / max_norm_value:
            raise ValueError(f'Value for normalization value {max_norm_value} probably too large with sigma_0 '
                             f'{sigma_0:.5f} and 1 / norm_value = {1. / max_norm_value}')

    # ------------------------------------------------------------------ schedule algebra (reference API)
    def phi(self, x, t, node_mask, edge_mask, context, mol_shape=None):
        """diffusion_qm9.py:135-138.  Differentiable when autograd is recording (see EGNN_dynamics_QM9._forward)."""
        return self.dynamics._forward(t, x, node_mask, edge_mask, context, mol_shape)

    def inflate_batch_array(self, array, target):
        return array.view((array.size(0),) + (1,) * (len(target.size()) - 1))

    def sigma(self, gamma, target_tensor):
        return self.inflate_batch_array(torch.sqrt(torch.sigmoid(gamma)), target_tensor)

    def alpha(self, gamma, target_tensor):
        return self.inflate_batch_array(torch.sqrt(torch.sigmoid(-gamma)), target_tensor)

    def SNR(self, gamma):
        return torch.exp(-gamma)

    def sigma_and_alpha_t_given_s(self, gamma_t, gamma_s, target_tensor):
        s2, s, a = sigma_and_alpha_t_given_s(gamma_t, gamma_s)
        return (self.inflate_batch_array(s2, target_tensor), self.inflate_batch_array(s, target_tensor),
                self.inflate_batch_array(a, target_tensor))

    def compute_x_pred(self, net_out, zt, gamma_t):
        sigma_t = self.sigma(gamma_t, target_tensor=net_out)
        alpha_t = self.alpha(gamma_t, target_tensor=net_out)
        return 1. / alpha_t * (zt - sigma_t * net_out)

    def unnormalize(self, x, h, node_mask):
        x = x * self.norm_values[0]
        h = (h * self.norm_values[1] + self.norm_biases[1]) * node_mask
        return x, h

    # ------------------------------------------------------------------ loss / NLL, forward value (reference API)
    # diffusion_qm9.py:160-172, 206-292, 460-751.  The network calls go through the HIP dynamics (per-row t); the
    # few element-wise terms around them are torch ops on the same device.  Under torch.no_grad() they return values
    # (validation NLL); with autograd recording they are differentiable (training_step): see `phi`.
    def subspace_dimensionality(self, node_mask):
        return (torch.sum(node_mask.squeeze(2), dim=1) - 1) * self.n_dims

    def normalize(self, x, h, node_mask):
        x = x / self.norm_values[0]
        delta_log_px = -self.subspace_dimensionality(node_mask) * math.log(self.norm_values[0])
        h = (h - self.norm_biases[1]) / self.norm_values[1] * node_mask
        return x, h, delta_log_px

    def _gamma_rows(self, t, key, gammas):
        """gamma at the [B,1] times `t`: fp64 evaluation rounded once (noise_model.evaluate_gamma) unless the caller
        replays recorded values (`gammas[key]`).  Every time the loss asks for lies on the grid k / T, k = -1 .. T
        (s = (t_int - 1) / T, t = t_int / T, 0, 1: diffusion_qm9.py:541-552), so without autograd the values come from a
        device-resident table of the T + 2 grid values - the same fp64 evaluation at the same fp32 arguments, tabulated
        once per version of the schedule parameters - and a loss evaluation needs no host round trip."""
        if gammas is not None and key in gammas:
            return torch.as_tensor(gammas[key], dtype=torch.float32, device=t.device).view(-1, 1)
        # training a LEARNED schedule: the network is part of the autograd graph (fp32, like the reference).  A predefined
        # schedule has no trainable parameter, and an evaluation call needs no graph: both read the table, so that the same
        # batch gives the same NLL whatever the grad mode
        if torch.is_grad_enabled() and self.training and any(p.requires_grad for p in self.gamma.parameters()):
            return self.gamma(t).view(-1, 1)
        gparams = list(self.gamma.state_dict(keep_vars=True).values())
        ver = (self.T, str(t.device), _lib.optimizer_generation()) + tuple((p.data_ptr(), p._version) for p in gparams)
        guard = self.__dict__.setdefault("_gamma_grid_guard", _lib.ImageGuard())
        if not guard.valid(ver, gparams):             # key AND content of the schedule parameters (_lib.ImageGuard)
            k = torch.arange(-1, self.T + 1, dtype=torch.float32).view(-1, 1)
            self._gamma_grid = evaluate_gamma(self.gamma, k / self.T).view(-1).to(t.device)
            guard.store(ver, gparams)
        idx = torch.round(t.to(torch.float32) * self.T).long().view(-1) + 1
        return self._gamma_grid[idx].view(-1, 1)

    def compute_error(self, net_out, gamma_t, eps):
        err = (eps - net_out) ** 2
        err = err.reshape(err.size(0), -1).sum(-1)
        if self.training and self.loss_type == 'l2':
            err = err / ((self.n_dims + self.in_node_nf) * net_out.shape[1])
        return err

    def kl_prior(self, xh, node_mask, gamma_T=None):
        B = xh.size(0)
        if gamma_T is None:
            gamma_T = self._gamma_rows(torch.ones((B, 1), device=xh.device), "gamma_T", None)
        nm = node_mask.to(xh.dtype)
        mu = self.alpha(gamma_T, xh) * xh
        sig = torch.sqrt(torch.sigmoid(gamma_T)).view(-1)
        sig3 = sig.view(-1, 1, 1)
        kl_h = ((torch.log(1.0 / sig3) + 0.5 * (sig3 ** 2 + mu[:, :, self.n_dims:] ** 2) - 0.5) * nm).reshape(B, -1).sum(-1)
        d = self.subspace_dimensionality(nm)
        mu2 = (mu[:, :, :self.n_dims] ** 2).reshape(B, -1).sum(-1)
        kl_x = d * torch.log(1.0 / sig) + 0.5 * (d * sig ** 2 + mu2) - 0.5 * d
        return kl_x + kl_h

    def log_constants_p_x_given_z0(self, x, node_mask, gamma_0=None):
        n_nodes = node_mask.squeeze(2).sum(1)
        if gamma_0 is None:
            gamma_0 = self._gamma_rows(torch.zeros((x.size(0), 1), device=x.device), "gamma_0", None)
        return (n_nodes - 1) * self.n_dims * (-0.5 * gamma_0.view(-1) - 0.5 * math.log(2 * math.pi))

    def log_constants_p_h_given_z0(self, h, node_mask, gamma_0=None):
        n_nodes = node_mask.squeeze(2).sum(1)
        if gamma_0 is None:
            gamma_0 = self._gamma_rows(torch.zeros((h.size(0), 1), device=h.device), "gamma_0", None)
        return n_nodes * self.in_node_nf * (-0.5 * gamma_0.view(-1) - 0.5 * math.log(2 * math.pi))

    def log_pxh_given_z0_without_constants(self, x, h, z_t, gamma_0, eps, net_out, node_mask, epsilon=1e-10):
        int_nf, cont_nf = (5, 3) if self.node_coarse_type == 'prop' else (3, 0)
        nd = self.n_dims
        z_h_int = z_t[:, :, nd:nd + int_nf]
        log_px = -0.5 * self.compute_error(net_out[:, :, :nd], gamma_0, eps[:, :, :nd])
        # the reference slices the continuous-feature prediction with a stride (`[: nd+int_nf : nd+int_nf+cont_nf]`,
        # diffusion_qm9.py:477), i.e. column 0 broadcast against the noise columns; kept for drop-in parity
        log_ph = -0.5 * self.compute_error(net_out[:, :, :nd + int_nf:nd + int_nf + cont_nf], gamma_0,
                                           eps[:, :, nd + int_nf:nd + int_nf + cont_nf])
        sigma_0_int = self.sigma(gamma_0, target_tensor=z_t) * self.norm_values[2]
        h_integer = torch.round(h[:, :, :int_nf] * self.norm_values[2] + self.norm_biases[2]).long()
        centred = h_integer - (z_h_int * self.norm_values[2] + self.norm_biases[2])
        cdf = lambda v: 0.5 * (1. + torch.erf(v / math.sqrt(2)))
        log_int = torch.log(cdf((centred + 0.5) / sigma_0_int) - cdf((centred - 0.5) / sigma_0_int) + epsilon)
        log_int = (log_int * node_mask).reshape(x.size(0), -1).sum(-1)
        return log_px + log_ph + log_int

    def compute_loss(self, x, h, node_mask, edge_mask, context, t0_always, mol_shape=None,
                     t_int=None, eps=None, eps0=None, gammas=None):
        """Forward value of the variational bound estimator / simple loss (diffusion_qm9.py:530-673).  Nodes behind
        `mol_shape` (pocket residues) are fixed: they enter the network un-noised and the loss covers the first
        mol_shape nodes (:553-579).  `t_int` [B,1], `eps`, `eps0` [B,mol,3+F] replay recorded draws (otherwise
        torch.randint / torch.randn on x.device, in the reference's order); `gammas` replays schedule values (keys
        gamma_s, gamma_t, gamma_0, gamma_T)."""
        B = x.size(0)
        dev = x.device
        mol = x.size(1) if mol_shape is None else int(mol_shape)
        x, x_fix = x[:, :mol], x[:, mol:]
        h, h_fix = h[:, :mol], h[:, mol:]
        node_mask_all = node_mask
        node_mask = node_mask[:, :mol]
        nm = node_mask.to(torch.float32)
        if t_int is None:
            t_int = torch.randint(1 if t0_always else 0, self.T + 1, size=(B, 1), device=dev).float()
        t_int = torch.as_tensor(t_int, dtype=torch.float32, device=dev).view(B, 1)
        s, t = (t_int - 1) / self.T, t_int / self.T
        t_is_zero = (t_int == 0).float().view(-1)
        if (gammas is None and x.is_cuda and torch.is_grad_enabled() and self.training
                and any(p.requires_grad for p in self.gamma.parameters())):
            # training a learned schedule: the four schedule values of the loss (diffusion_qm9.py:541-552) from ONE pass of the
            # network over [s; t; 0; 1] instead of four (each ~125 small launches forward + backward)
            gamma_s, gamma_t, gamma_0, gamma_T = self.gamma(torch.cat([s, t, torch.zeros_like(t), torch.ones_like(t)], dim=0)).view(4, B, 1)
        else:
            gamma_s, gamma_t = self._gamma_rows(s, "gamma_s", gammas), self._gamma_rows(t, "gamma_t", gammas)
            gamma_0 = self._gamma_rows(torch.zeros_like(t), "gamma_0", gammas)
            gamma_T = self._gamma_rows(torch.ones_like(t), "gamma_T", gammas)
        if eps is None:
            eps = self.sample_combined_position_feature_noise(B, mol, node_mask)
        eps = torch.as_tensor(eps, dtype=torch.float32, device=dev)
        xh = torch.cat([x, h], dim=2).to(torch.float32)
        if (self.fused_loss and not t0_always and mol_shape is None and x.is_cuda and torch.is_grad_enabled() and self.training
                and xh.shape[2] == self.n_dims + self.in_node_nf):
            # the training loss around the network call as one launch per direction (training.vlb_zt / vlb_loss, csrc/k_loss.hpp);
            # everything this branch skips below is the same arithmetic in ~350 element-wise launches, kept for every other case
            # (evaluation, pocket models, CPU) and as the oracle of tests/test_gpu_training.py
            from .training import vlb_loss, vlb_zt
            self._check_mean_zero(x, node_mask)
            gam = torch.stack([gamma_s.reshape(B), gamma_t.reshape(B), gamma_0.reshape(B), gamma_T.reshape(B)])
            xh, eps = xh.contiguous(), eps.contiguous()
            z_t = vlb_zt(xh, eps, gam[1])
            net_out = self.phi(z_t, t, node_mask_all, edge_mask, context, mol_shape=mol)
            int_nf, cont_nf = (5, 3) if self.node_coarse_type == 'prop' else (3, 0)
            l2_train = self.loss_type == 'l2'
            consts = (int_nf, cont_nf, l2_train, float(self.T), float(self.norm_values[2]), float(self.norm_biases[2]), 0.0)
            loss, error = vlb_loss(net_out, z_t, gam, xh, eps, nm.reshape(B, mol).contiguous(), t_int.reshape(B).contiguous(), consts)
            return loss, {'t': t_int.squeeze(), 'loss_t': loss.squeeze(), 'error': error.squeeze()}
        xh_fix = torch.cat([x_fix, h_fix], dim=2).to(torch.float32)
        self._check_mean_zero(x, node_mask)
        z_t = self.alpha(gamma_t, x) * xh + self.sigma(gamma_t, x) * eps
        self._check_mean_zero(z_t[:, :, :self.n_dims], node_mask)
        z_t = torch.cat([z_t, xh_fix], dim=1)
        net_out = self.phi(z_t, t, node_mask_all, edge_mask, context, mol_shape=mol)[:, :mol]
        error = self.compute_error(net_out, gamma_t, eps)
        l2_train = self.training and self.loss_type == 'l2'
        snr_weight = torch.ones_like(error) if l2_train else (self.SNR(gamma_s - gamma_t) - 1).view(-1)
        loss_t_larger_than_zero = 0.5 * snr_weight * error
        neg_log_constants = -self.log_constants_p_x_given_z0(x, nm, gamma_0) - self.log_constants_p_h_given_z0(h, nm, gamma_0)
        if l2_train:
            neg_log_constants = torch.zeros_like(neg_log_constants)
        kl_prior = self.kl_prior(xh, nm, gamma_T)
        if t0_always:
            if eps0 is None:
                eps0 = self.sample_combined_position_feature_noise(B, mol, node_mask)
            eps0 = torch.as_tensor(eps0, dtype=torch.float32, device=dev)
            z_0 = torch.cat([self.alpha(gamma_0, x) * xh + self.sigma(gamma_0, x) * eps0, xh_fix], dim=1)
            net0 = self.phi(z_0, torch.zeros_like(t), node_mask_all, edge_mask, context, mol_shape=mol)[:, :mol]
            loss_term_0 = -self.log_pxh_given_z0_without_constants(x, h, z_0[:, :mol], gamma_0, eps0, net0, nm)
            loss = kl_prior + self.T * loss_t_larger_than_zero + neg_log_constants + loss_term_0
        else:
            loss_term_0 = -self.log_pxh_given_z0_without_constants(x, h, z_t[:, :mol], gamma_t, eps, net_out, nm)
            loss_t = loss_term_0 * t_is_zero + (1 - t_is_zero) * loss_t_larger_than_zero
            estimator = loss_t if l2_train else (self.T + 1) * loss_t
            loss = kl_prior + estimator + neg_log_constants
        return loss, {'t': t_int.squeeze(), 'loss_t': loss.squeeze(), 'error': error.squeeze()}

    def nll(self, x, h, node_mask=None, edge_mask=None, context=None, mol_shape=None, **replay):
        """Loss if training (value only), NLL estimate if eval (diffusion_qm9.py:675-699)."""
        x, h, delta_log_px = self.normalize(x, h, node_mask.to(torch.float32))
        if self.training and self.loss_type == 'l2':
            delta_log_px = torch.zeros_like(delta_log_px)
        loss, _ = self.compute_loss(x, h, node_mask, edge_mask, context, t0_always=not self.training,
                                    mol_shape=mol_shape, **replay)
        return loss - delta_log_px

    def forward(self, batch, **replay):
        """`{"loss": mean NLL}` for a reference data batch (keys positions, atom_mask, edge_mask, node_feature; with a
        context model, context; with a pocket model, protein_pos, protein_feat, protein_feat_mask,
        protein_edge_mask) - diffusion_qm9.py:701-751."""
        x, node_mask, edge_mask, h = batch['positions'], batch['atom_mask'], batch['edge_mask'], batch["node_feature"]
        mol_shape = None
        if self.pocket:
            mol_shape = x.shape[1]
            x = torch.cat([x, batch["protein_pos"].to(x.dtype)], dim=1)
            node_mask = torch.cat([node_mask, batch["protein_feat_mask"]], dim=1)
            P = batch["protein_edge_mask"].shape[1]
            em = torch.zeros(edge_mask.shape[0], mol_shape + P, mol_shape + P, dtype=edge_mask.dtype, device=edge_mask.device)
            em[:, :mol_shape, :mol_shape] = edge_mask.view(-1, mol_shape, mol_shape)
            em[:, mol_shape:, mol_shape:] = batch["protein_edge_mask"]
            edge_mask = em
            h = torch.cat([h, self.pocket_embed(batch["protein_feat"]).to(h.dtype)], dim=1)
        nm = node_mask.to(x.dtype)
        if self.debug_checks:                       # models/utils.py:47-50
            bad = (x * (1 - nm)).abs().sum().item()
            assert bad < 1e-5, f'Error {bad} too high'
        fix = x.size(1) if mol_shape is None else mol_shape
        # remove_mean_with_mask(x, node_mask, fix_size=mol_shape): the mean of the first mol_shape nodes is taken off
        # every valid node, pocket residues included (models/utils.py:51-56)
        x = x - (x[:, :fix].sum(1, keepdim=True) / nm[:, :fix].sum(1, keepdim=True)) * nm
        context = batch['context'] if self.dynamics.context_node_nf > 0 else None
        if context is not None and self.training and self.context_drop_prob > 0:
            from . import guidance
            context = guidance.drop_context(context, self.context_drop_prob, self.null_context, node_mask, self.context_drop_generator)
        bs, n_nodes, _ = x.size()
        edge_mask = edge_mask.reshape(bs, n_nodes * n_nodes)
        self._check_masked(x, node_mask, "assert_correctly_masked")
        neg_log_pxh = self.nll(x, h, node_mask, edge_mask, context=context, mol_shape=mol_shape, **replay)
        return {"loss": neg_log_pxh.mean(0)}

    def stage_batch(self, batch, device=None):
        """A collated HOST batch (the dict a DataLoader yields) -> the device batch `forward` / `training_step` take, without
        a host wait: tensors travel through pinned copies in stream order, and the masks' topology is laid out from the
        host copies on the way (`EGNN_dynamics_QM9.stage_masks`) - so a loop that stages batch k+1 after launching step k
        overlaps the layout with the GPU's work.  This is the place of Lightning's transfer_batch_to_device in the reference's
        trainer.  Pocket batches (their masks are composed on the device in `forward`) and tensors already on the device
        are moved as they are."""
        from .dynamics import _to_device_async
        dev = self.dynamics._device() if device is None else torch.device(device)
        out = {k: (_to_device_async(v, dev) if torch.is_tensor(v) else v) for k, v in batch.items()
               if k not in ("atom_mask", "edge_mask")}
        nm, em = batch.get("atom_mask"), batch.get("edge_mask")
        if (not self.pocket and torch.is_tensor(nm) and nm.device.type == "cpu"
                and (em is None or (torch.is_tensor(em) and em.device.type == "cpu"))):
            nm_d, em_d = self.dynamics.stage_masks(nm, em, dev)
            out["atom_mask"] = nm_d
            if "edge_mask" in batch:
                out["edge_mask"] = em_d
        else:
            for k in ("atom_mask", "edge_mask"):
                if k in batch:
                    out[k] = _to_device_async(batch[k], dev) if torch.is_tensor(batch[k]) else batch[k]
        return out

    def training_step(self, batch, batch_idx=0):
        """diffusion_qm9.py:774-777: differentiable mean loss of the batch (call .backward() on it, then - multi-GPU -
        hierdiff_amd.sharding.allreduce_gradients, the DDP step of conf/trainer/default.yaml:2-3)."""
        loss = self.forward(batch)["loss"]
        if hasattr(self, "log") and _Base is not nn.Module:
            self.log("train_loss", loss, on_epoch=True, prog_bar=True)
        return loss

    @torch.no_grad()
    def validation_step(self, batch, batch_idx=0):
        """diffusion_qm9.py:779-781 (value only)."""
        return self.forward(batch)

    test_step = validation_step

    # ------------------------------------------------------------------ epoch-end hooks and optimiser (Lightning side of the module)
    # diffusion_qm9.py:753-801, 871-879.  With pytorch_lightning installed the base class provides `log`, `all_gather`,
    # `global_rank`; without it (this image) the same hooks work over torch.distributed, or on one process.
    def _rank(self) -> int:
        if _Base is not nn.Module:
            return int(self.global_rank)
        import torch.distributed as dist
        return dist.get_rank() if dist.is_available() and dist.is_initialized() else 0

    def _gather_ranks(self, value: torch.Tensor) -> torch.Tensor:
        """[world, ...] stack of `value` from every rank (LightningModule.all_gather's shape; [1, ...] on one process).  Every
        rank must hold the same shape, as under Lightning."""
        if _Base is not nn.Module:
            out = self.all_gather(value)
            return out if out.dim() > value.dim() else out.unsqueeze(0)
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
            return value.unsqueeze(0)
        parts = [torch.empty_like(value) for _ in range(dist.get_world_size())]
        dist.all_gather(parts, value.contiguous())
        return torch.stack(parts)

    def _gather_result(self, result):
        """List of per-step dicts -> one dict of tensors: first the steps are joined (tensors concatenated, scalars stacked into
        a vector), then the ranks (diffusion_qm9.py:753-766)."""
        keys = list(result[0].keys())
        steps = {}
        for key in keys:
            first = result[0][key]
            if first.dim() > 0:
                steps[key] = torch.cat([r[key] for r in result])
            else:
                steps[key] = torch.stack([r[key].detach() for r in result]).to(first)
        return {key: torch.cat(list(self._gather_ranks(steps[key]))) for key in keys}

    def _compute_metrics(self, result):
        """diffusion_qm9.py:768-772: the epoch metric is the mean of the gathered per-step losses."""
        return {'loss': result['loss'].mean()}

    def _log(self, name, value, **kw):
        if _Base is not nn.Module:
            self.log(name, value, **kw)
        else:                                   # no Lightning: the last logged values stay readable on the module
            self.logged = getattr(self, "logged", {})
            self.logged[name] = value

    def validation_epoch_end(self, result):
        """diffusion_qm9.py:787-795."""
        metrics = self._compute_metrics(self._gather_result(result))
        self._log("val_loss", metrics["loss"], on_epoch=True, prog_bar=True)

    def test_epoch_end(self, result):
        """diffusion_qm9.py:797-800 (logged by rank 0 only)."""
        metrics = self._compute_metrics(self._gather_result(result))
        if self._rank() == 0:
            self._log("test/ppl", metrics["loss"], on_epoch=True)

    def configure_optimizers(self):
        """diffusion_qm9.py:871-879: `[optimizer], [scheduler]` from `cfg.optim` / `cfg.scheduler` (hydra nodes with a `_target_`,
        conf/optim/adamw.yaml, conf/scheduler/step.yaml).  hydra's `instantiate` is used when the package exists; otherwise the
        `_target_` is resolved here - only names under `torch.optim` are accepted - and a cfg without these nodes gets the
        reference's shipped values (AdamW 4e-4 / 4e-8, StepLR 15 / 0.1: hierdiff_amd.trainer.configure_optimizers, fused update
        on the GPU).  A scheduler node that asks for `num_training_steps` needs the Lightning trainer and is not supported
        without it."""
        from .trainer import configure_optimizers as _defaults
        optim_cfg, sched_cfg = _get(self.cfg, "optim", None), _get(self.cfg, "scheduler", None)
        if optim_cfg is None:
            opt, sched = _defaults(self)
            if sched_cfg is not None:
                sched = self._instantiate(sched_cfg, opt)
            return [opt], [sched]
        opt = self._instantiate(optim_cfg, self.parameters())
        sched = self._instantiate(sched_cfg, opt) if sched_cfg is not None else torch.optim.lr_scheduler.StepLR(opt, step_size=15, gamma=0.1)
        return [opt], [sched]

    @staticmethod
    def _instantiate(node, *args):
        node = dict(node)
        if "num_training_steps" in node:
            raise NotImplementedError("schedulers keyed on num_training_steps need the Lightning trainer (diffusion_qm9.py:804-869)")
        try:
            from hydra.utils import instantiate  # type: ignore
            return instantiate(node, *args)
        except ImportError:
            pass
        target = str(node.pop("_target_"))
        if not target.startswith("torch.optim."):
            raise ValueError(f"_target_ {target!r}: only torch.optim.* optimisers / lr_schedulers are resolved without hydra")
        obj = torch.optim
        for part in target.split(".")[2:]:
            obj = getattr(obj, part)
        return obj(*args, **node)

    # ------------------------------------------------------------------ HIP plumbing
    def _lib_handle(self, synced: bool = False):
        """The dynamics' handle with its weight image confirmed (key + content digest, `sync_weights`).  `synced`: the caller has just
        evaluated the network through this handle (`phi`), which confirmed it - the check costs a stream wait, and the step-by-step
        samplers would pay it twice per diffusion step."""
        if not (synced and getattr(self.dynamics, "mode", "egnn_dynamics") == "egnn_dynamics"):
            self.dynamics.sync_weights()
        return self.dynamics._handle()

    def _schedule(self, rows: int = 1):
        """Tabulated schedule, uploaded to the handle (hd_set_schedule); recomputed when gamma changes."""
        handle = self._lib_handle()          # creates the handle if needed: its generation is part of the key (a new
        # handle - other precision, other device - has no schedule yet, even if it re-uses a freed handle's address)
        key = (self.T, self.dynamics._handle_gen, _lib.optimizer_generation()) + tuple(
            (p.data_ptr(), p._version) for p in self.gamma.parameters()) + (
                id(self.schedule_gammas), self.schedule_eval, rows if self.schedule_eval == "fp32" else 0)
        gparams = list(self.gamma.parameters())
        guard = self.__dict__.setdefault("_sched_guard", _lib.ImageGuard())
        if self._sched_key is None:
            guard.clear()
        if not guard.valid(key, gparams):             # key AND content of the schedule parameters (_lib.ImageGuard)
            tabs = schedule_tables(self.gamma, self.T, self.schedule_gammas, self.schedule_eval, rows)
            tau = tabs["tau"].numpy().astype(np.float32)
            coef = tabs["coef"].numpy().astype(np.float32).reshape(-1)
            _lib.check(_lib.load().hd_set_schedule(
                handle, self.T, tau.ctypes.data_as(C.POINTER(C.c_float)),
                coef.ctypes.data_as(C.POINTER(C.c_float))), "hd_set_schedule")
            self._sched = tabs
            guard.store(key, gparams)
            self._sched_key = key
        return self._sched

    def _plan(self, what: str, kind: str = "full", fix_noise: bool = False, **kw):
        """The host side of the sampling call `what` (`plan.plan`): its keywords resolved once, before the GPU is touched.
        `fix_noise`: the call shares one row of noise, which a steered plan refuses."""
        pl = make_plan(self, what, kind, **kw)
        if pl.steer is not None and fix_noise:
            raise ValueError(f"{what}: steering needs every row's own noise (fix_noise shares one row: duplicated particles would "
                             "never diverge)")
        if pl.diversity is not None and fix_noise:
            if diversity_mod.stochastic(pl.eta):
                raise ValueError(f"{what}: diversity with fix_noise is allowed only on a path that draws nothing (eta = 0, solver "
                                 "'dpm2m'): shared noise would pull the rows of a group together again")
        if pl.corrector is not None and pl.diversity is not None and fix_noise:
            raise ValueError(f"{what}: diversity with fix_noise is allowed only on a call that draws nothing, and corrector steps draw: "
                             "shared noise would pull the rows of a group together again")
        return pl

    def _resolve_path(self, steps=None, eta=None, spacing=None, timesteps=None, inpaint: bool = False, solver=None,
                      lower_order_final=None):
        """The path keywords alone (None: the model's `sample_*` attributes) -> None for the plain loop, or (path, eta); with solver
        "dpm2m" (path, `paths.Multistep`).  A view of `plan.full_path`."""
        return full_path(self, steps, eta, spacing, timesteps, inpaint, solver, lower_order_final)

    def _upload_path(self, tabs, key, build, upload):
        """The path tables on the handle, cached per (schedule table, key): `build()` computes them, `upload(tables)` sets them.  One
        cache for both directions (hd_set_path / hd_set_path_multistep and hd_set_path_up fill the same tables): whichever was set
        last is the one that is cached.  `_rows_open` keys the uploads of the loop terms on the identity of the cached tables."""
        hit = self.__dict__.get("_path_cache")
        if hit is None or hit[0] is not tabs or hit[1] != key:
            pt = build()
            self._path_cache = None
            upload(pt)
            self._path_cache = (tabs, key, pt)
        return self._path_cache[2]

    def _path_tables(self, handle, tabs, path, eta):
        """Rows of `path` from the gamma grid of `_schedule`, uploaded to the handle (hd_set_path; hd_set_path_multistep when `eta`
        is a `paths.Multistep`) once per (table, path, eta or solver with its lower_order_final)."""
        from . import paths
        ms = isinstance(eta, paths.Multistep)
        ip, fp = (lambda a: np.ascontiguousarray(a.numpy(), dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int)),
                  lambda a: None if a is None else np.ascontiguousarray(a.numpy(), dtype=np.float32).ctypes.data_as(C.POINTER(C.c_float)))

        def upload(pt):
            if ms and eta.stochastic:
                _lib.check(_lib.load().hd_set_path_multistep_sde(handle, pt["K"], ip(pt["t_idx"]), ip(pt["s_idx"]), fp(pt["coef"])),
                           "hd_set_path_multistep_sde")
            elif ms:
                _lib.check(_lib.load().hd_set_path_multistep(handle, pt["K"], ip(pt["t_idx"]), ip(pt["s_idx"]), fp(pt["coef"])),
                           "hd_set_path_multistep")
            else:
                _lib.check(_lib.load().hd_set_path(handle, pt["K"], ip(pt["t_idx"]), ip(pt["s_idx"]), fp(pt["coef"]), pt["form"],
                                                   fp(pt["coef_inpaint"])), "hd_set_path")

        return self._upload_path(tabs, (tuple(path), ("sde2m" if eta.stochastic else "dpm2m", bool(eta.lower_order_final)) if ms else float(eta)),
                                 lambda: paths.path_tables(tabs["gamma"], path, eta), upload)

    # ------------------------------------------------------------------ what a call attaches to its topology (the loop terms)
    def _rows_open(self, name: str, key, build, setter: str):
        """The per-transition rows of the loop term `name`, behind the path tables `_path_tables` has just set: `build(pt)` gives the
        arguments of the library's `setter`.  Once per (path tables, key): `_row_caches[name]` holds what was uploaded last."""
        pt = self._path_cache[2]
        caches = self.__dict__.get("_row_caches") or {}
        hit = caches.get(name)
        if hit is None or hit[0] is not pt or hit[1] != key:
            args = build(pt)
            caches.pop(name, None)
            _lib.check(getattr(_lib.load(), setter)(*args), setter)
            caches[name] = (pt, key)
        self._row_caches = caches

    @staticmethod
    def _row_args(handle, tabs, pt, rows_of):
        """(handle, K, rows [K, w] float32) for a row setter: `rows_of(gamma, path)` on the grid indices of the path tables `pt`."""
        rows = np.ascontiguousarray(rows_of(tabs["gamma"], [int(t) for t in pt["t_idx"]] + [int(pt["s_idx"][-1])]))
        return handle, int(rows.shape[0]), rows.ctypes.data_as(C.POINTER(C.c_float))

    def _chain_open(self, handle, topo, tabs, cf, what: int, B: int, N: int, dev, chain=None):
        """The sink [keep, B, N, D] of a recording call (`chain`: the one an earlier piece of the same chain wrote to), attached to
        `topo` (hd_chain_attach) behind the path's frame table (hd_set_chain, once per (path tables, frame table)).  The caller detaches."""
        keep = len(cf.frame_t)

        def build(pt):
            als = np.ascontiguousarray([self._alpha_sigma(tabs, int(t)) for t in pt["t_idx"]], dtype=np.float32)
            fo = np.ascontiguousarray(cf.frame_of, dtype=np.int32)
            return handle, int(fo.shape[0]), fo.ctypes.data_as(C.POINTER(C.c_int)), als.ctypes.data_as(C.POINTER(C.c_float)), keep
        self._rows_open("chain", (tuple(cf.frame_of), keep), build, "hd_set_chain")
        if chain is None:
            chain = torch.zeros((keep, B, N, self.n_dims + self.in_node_nf), device=dev, dtype=torch.float32)
        _lib.check(_lib.load().hd_chain_attach(topo.ptr, chain.data_ptr(), keep, int(what), float(self.norm_values[0]),
                                               float(self.norm_values[1]), float(self.norm_biases[1] or 0.0)), "hd_chain_attach")
        return chain

    def _restrain_open(self, handle, topo, tabs, rr, B: int, dev):
        """Attach the restraints of a resolved call (`restraints.Resolved`) to `topo` behind their rows (hd_set_restraint, once per
        (path tables, schedule, clip)).  The caller detaches (`Restraints.detach`)."""
        nv0, nv1 = float(self.norm_values[0]), float(self.norm_values[1])
        self._rows_open("restraint", rr.key(), lambda pt: self._row_args(
            handle, tabs, pt, lambda g, path: restraints_mod.lambda_rows(g, path, rr.schedule, rr.clip, nv0)), "hd_set_restraint")
        rr.rs.check_batch(B)
        import weakref
        rr.rs._model = weakref.ref(self)
        rr.rs.attach(topo, rr.scale, nv0, dev, _stream(dev), rr.frame,
                     feat=(nv1, float(self.norm_biases[1] or 0.0), restraints_mod.feature_ratio(rr.schedule, nv0, nv1)))

    def _steer_open(self, handle, topo, tabs, st, reset: bool, dev):
        """Attach the steering of a resolved call (`steering.Steer`) to `topo` behind its rows (hd_set_steer, once per (path tables,
        beta, schedule)).  `reset`: the call starts a chain (k_lo = 0), else it continues.  The caller closes (`steering.close`)."""
        self._rows_open("steer", st.key(), lambda pt: self._row_args(handle, tabs, pt, lambda g, path: steering_mod.beta_rows(g, path, st)),
                        "hd_set_steer")
        steering_mod.attach(topo, st, reset, _stream(dev))

    def _diversity_open(self, handle, topo, tabs, dv, dev):
        """Attach the diversity of a resolved call (`diversity.Diversity`) to `topo` behind its rows (hd_set_diversity, once per (path
        tables, schedule, clip)).  The caller detaches (hd_diversity_detach)."""
        nv0 = float(self.norm_values[0])
        self._rows_open("diversity", dv.key(), lambda pt: self._row_args(handle, tabs, pt, lambda g, path: diversity_mod.rows(g, path, dv, nv0)),
                        "hd_set_diversity")
        diversity_mod.attach(topo, dv.P, dv.strength, dv.length, dv.scale, nv0, _stream(dev))

    def _corrector_open(self, handle, topo, tabs, cr, dev):
        """Attach the corrector of a resolved call (`corrector.Corrector`) to `topo` behind its rows (hd_set_corrector, once per (path
        tables, mode, strength, cap)).  The caller detaches (hd_corrector_detach)."""
        self._rows_open("corrector", cr.key(), lambda pt: self._row_args(handle, tabs, pt, lambda g, path: corrector_mod.rows(g, path, cr)),
                        "hd_set_corrector")
        corrector_mod.attach(topo, cr, _stream(dev))

    def _diversity_result(self, pl, x, node_mask):
        """`diversity_last` of a diverse call's returned x: Phi and the aligned RMSD matrix per group (hd_diversity_energy), attached as
        the call attached it, so its cached graph stays."""
        dv = getattr(pl, "diversity", None)
        if dv is None:
            return
        phi, rmsd = diversity_mod._device_energy(x, node_mask, dv.P, dv.length, dv.strength, self, "diversity",
                                             _attach=(dv.scale, float(self.norm_values[0])))
        self.diversity_last = diversity_mod.result(phi, rmsd)

    def _chain_times(self, keep_frames, t_start=None, inpaint: bool = False, **few):
        """[keep] the grid index every frame of a recording call has arrived at (`Plan.chain_t`): host arithmetic only."""
        kind = "latent" if t_start is not None else "inpaint" if inpaint else "full"
        return self._plan("chain", kind, t_start=t_start, keep_frames=keep_frames, **few).chain_t

    def _chain_into(self, results, chain, sizes, chain_t):
        """'chain_x' [keep, n_i, 3], 'chain_h' [keep, n_i, F], 'chain_t' [keep] into every molecule's dict (CPU, trimmed)."""
        c = chain.cpu()
        for i, res in enumerate(results):
            n = int(sizes[i])
            res['chain_x'] = c[:, i, :n, :self.n_dims].clone()
            res['chain_h'] = c[:, i, :n, self.n_dims:].clone()
            res['chain_t'] = chain_t.clone()
        return results

    def _restraint_entries(self, rs, scale, x, node_mask, fixed_mask=None, x_known=None, cpu: bool = True, h=None) -> dict:
        """`Restraints.result_entries` of a restrained call's returned x (and h: the feature entries), attached as the call attached
        them (its scales, the model's nv0); `cpu`: moved to the CPU."""
        ent = rs.result_entries(x, node_mask, self, (torch.as_tensor(scale), float(self.norm_values[0])), fixed_mask, x_known, h=h)
        return {k: v.cpu() for k, v in ent.items()} if cpu else ent

    def _check_masked(self, x, node_mask, what):
        if self.debug_checks:
            bad = (x * (~node_mask.bool())).abs().max().item()
            assert bad < 1e-4, f'{what}: variables not masked properly ({bad})'

    def _check_mean_zero(self, x, node_mask):
        if self.debug_checks:
            self._check_masked(x, node_mask, "assert_mean_zero_with_mask")
            largest = x.abs().max().item()
            err = torch.sum(x, dim=1, keepdim=True).abs().max().item()
            assert err / (largest + 1e-10) < 1e-2, f'Mean is not zero, relative_error {err / (largest + 1e-10)}'

    # ------------------------------------------------------------------ single transitions (reference API)
    def sample_combined_position_feature_noise(self, n_samples, n_nodes, node_mask):
        """diffusion_qm9.py:445-456 with torch.randn draws on node_mask.device (x first, then h)."""
        dev = node_mask.device
        nm = node_mask.to(torch.float32)
        raw_x = torch.randn((n_samples, n_nodes, self.n_dims), device=dev)
        raw_h = torch.randn((n_samples, n_nodes, self.in_node_nf), device=dev)
        zx = raw_x * nm
        zx = zx - (zx.sum(1, keepdim=True) / nm.sum(1, keepdim=True)) * nm
        return torch.cat([zx, raw_h * nm], dim=2)

    def _combine_raw(self, raw, node_mask, B):
        """z_T from an injected (randn_x [b,N,3], randn_h [b,N,F]) pair: masked, x centred (diffusion_qm9.py:445-456), b = 1 broadcast."""
        dev = node_mask.device
        nm = node_mask.to(torch.float32)
        rx, rh = (r.to(dev, torch.float32) for r in raw)
        zx = rx * nm
        zx = zx - (zx.sum(1, keepdim=True) / nm.sum(1, keepdim=True)) * nm
        z = torch.cat([zx, rh * nm], dim=2)
        return z.expand(B, -1, -1).contiguous() if z.shape[0] == 1 and B > 1 else z.contiguous()

    @torch.no_grad()
    def sample_p_zs_given_zt(self, s, t, zt, node_mask, edge_mask, context, fix_noise=False, mol_shape=None,
                             raw_noise: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
                             gammas: Optional[Tuple[torch.Tensor, torch.Tensor]] = None):
        """zs ~ p(zs | zt) (diffusion_qm9.py:312-345).  Returns [B, mol_shape, D]: the reference
        appends an empty slice because `zt` was re-bound to its first mol_shape nodes (:326,:345).
        raw_noise / gammas optionally inject the two randn draws / (gamma_s, gamma_t)."""
        dev = zt.device
        B, N, D = zt.shape
        mol = N if mol_shape is None else min(int(mol_shape), N)
        if gammas is None:
            gammas = (evaluate_gamma(self.gamma, s), evaluate_gamma(self.gamma, t))
        coef = step_coefficients(gammas[0].detach().float().cpu().reshape(-1, 1),
                                 gammas[1].detach().float().cpu().reshape(-1, 1)).to(dev)
        zt_c = zt.detach().to(torch.float32).contiguous()
        eps = self.phi(zt_c, t, node_mask, edge_mask, context, mol_shape)
        self._check_mean_zero(zt_c[:, :mol, :self.n_dims], node_mask[:, :mol])
        nb = 1 if fix_noise else B
        if raw_noise is None:
            raw_x = torch.randn((nb, mol, self.n_dims), device=dev)
            raw_h = torch.randn((nb, mol, self.in_node_nf), device=dev)
        else:
            raw_x, raw_h = (r.to(dev, torch.float32).contiguous() for r in raw_noise)
        topo = self.dynamics.topology(node_mask, edge_mask, B, N)
        zs = torch.empty((B, mol, D), device=dev, dtype=torch.float32)
        _lib.check(_lib.load().hd_posterior_step(
            self._lib_handle(synced=True), topo.ptr, zt_c.data_ptr(), eps.data_ptr(), coef.data_ptr(), coef.shape[0],
            raw_x.data_ptr(), raw_h.data_ptr(), raw_x.shape[0], mol, zs.data_ptr(), _stream(dev)), "hd_posterior_step")
        return zs

    @torch.no_grad()
    def sample_p_xh_given_z0(self, z0, node_mask, edge_mask, context, fix_noise=False,
                             raw_noise: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
                             gamma_0: Optional[torch.Tensor] = None):
        """x ~ p(x | z0), h = z0 features (diffusion_qm9.py:294-310)."""
        dev = z0.device
        B, N, D = z0.shape
        zeros = torch.zeros(size=(B, 1), device=dev)
        if gamma_0 is None:
            gamma_0 = evaluate_gamma(self.gamma, torch.zeros(1, 1))
        z0_c = z0.detach().to(torch.float32).contiguous()
        eps = self.phi(z0_c, zeros, node_mask, edge_mask, context)
        coef3 = decode_coefficients(gamma_0.detach().float().cpu()).numpy()
        return self._final_decode(z0_c, eps, node_mask, edge_mask, coef3, fix_noise, raw_noise)

    def _final_decode(self, z0, eps, node_mask, edge_mask, coef3, fix_noise, raw_noise, philox=None):
        """raw_noise: (randn_x, randn_h) or None -> torch.randn; philox=(sample_id_base, draw) uses the
        library's counter RNG instead."""
        dev = z0.device
        B, N, D = z0.shape
        nb = 1 if fix_noise else B
        raw_x = raw_h = None
        if philox is None:
            if raw_noise is None:
                raw_x = torch.randn((nb, N, self.n_dims), device=dev)
                raw_h = torch.randn((nb, N, self.in_node_nf), device=dev)
            else:
                raw_x, raw_h = (r.to(dev, torch.float32).contiguous() for r in raw_noise)
            nb = raw_x.shape[0]
        topo = self.dynamics.topology(node_mask, edge_mask, B, N)
        x = torch.empty((B, N, self.n_dims), device=dev, dtype=torch.float32)
        h = torch.empty((B, N, self.in_node_nf), device=dev, dtype=torch.float32)
        c3 = np.ascontiguousarray(coef3, dtype=np.float32)
        _lib.check(_lib.load().hd_final_decode(
            self._lib_handle(synced=True), topo.ptr, z0.data_ptr(), eps.data_ptr(), c3.ctypes.data_as(C.POINTER(C.c_float)),
            _ptr(raw_x), _ptr(raw_h), nb, self.seed, philox[0] if philox else 0, philox[1] if philox else 0,
            int(fix_noise), x.data_ptr(), h.data_ptr(), _stream(dev)), "hd_final_decode")
        if not self._unit_norm:         # `unnormalize` (:174-179); h is already masked: (h nv1 + nb1) mask = h_masked nv1 + nb1 mask
            x = x * float(self.norm_values[0])
            h = h * float(self.norm_values[1]) + float(self.norm_biases[1] or 0.0) * node_mask.reshape(B, N, 1).to(h.dtype)
        return x, h

    def sample_normal(self, mu, sigma, node_mask, fix_noise=False):
        bs = 1 if fix_noise else mu.size(0)
        return mu + sigma * self.sample_combined_position_feature_noise(bs, mu.size(1), node_mask)

    # ------------------------------------------------------------------ classifier-free guidance (no reference counterpart)
    def _guide_device(self, gd, node_mask, dev):
        """Device-side inputs of a guided call: (null / second context rows [B*N,C], scales [rows], rows, phi)."""
        from . import guidance
        B, N = int(node_mask.shape[0]), int(node_mask.shape[1])
        C_ = int(self.dynamics.context_node_nf)
        if gd.context is None:
            ctx_u = guidance.masked_null_context(self.null_context, node_mask.to(dev), C_)
        else:
            ctx_u = gd.context.to(dev, torch.float32)
        return AttrDict(ctx_u=ctx_u.reshape(B * N, C_).contiguous(), w=gd.w.to(dev).contiguous(), rows=gd.rows, phi=gd.rescale)

    def _decode_eps(self, topo, z, ctx, g=None):
        """The network call of the final decode (t = 0); guided the way the loop's calls are: two forwards, hd_guide_combine."""
        dev = z.device
        zeros = torch.zeros((z.shape[0], 1), device=dev)
        eps = self.dynamics.forward_with_topology(topo, zeros, z, ctx, None)
        if g is None:
            return eps
        eps_u = self.dynamics.forward_with_topology(topo, zeros, z, g.ctx_u, None)
        _lib.check(_lib.load().hd_guide_combine(self._lib_handle(synced=True), topo.ptr, eps.data_ptr(), eps_u.data_ptr(),
                                                g.w.data_ptr(), g.rows, g.phi, eps.data_ptr(), _stream(dev)), "hd_guide_combine")
        return eps

    # ------------------------------------------------------------------ the three device steps of every sampling call
    def _device_state(self, node_mask, edge_mask, context, B, N, pl=None, what: str = "sampling", needs_context: bool = True,
                      inpaint: bool = False):
        """The first lines of a call that need the GPU: handle, schedule (`inpaint`: with the inpainting rows), the tables of the
        plan's path, topology, context rows [B*N, C] and the guided call's second context.  Entry points add their extras (pocket:
        `tail`, `topo_loop`; inpainting: `_inpaint_setup`) on top of it."""
        dev = node_mask.device
        if pl is not None and pl.steer is not None:   # rows of a group interact: equal masks, contexts and tables, checked on the host
            steering_mod.check_groups(pl.steer, node_mask, context, pl.restraints.rs, pl.restraints.scale, what)
        if pl is not None and pl.diversity is not None:
            diversity_mod.check_groups(pl.diversity, node_mask, context, what)
        if dev.type != "cuda":
            raise _lib.HierDiffHipError(f"{what} runs only on an MI355X (no CPU fallback)")
        h = self._lib_handle()
        tabs = self._schedule(rows=B)
        if inpaint:
            self._inpaint_schedule(h, tabs)
        if pl is not None and pl.path is not None:
            self._path_tables(h, tabs, pl.path, pl.eta)
        topo = self.dynamics.topology(node_mask, edge_mask, B, N)
        ctx = None
        if self.dynamics.context_node_nf > 0 and (needs_context or context is not None):
            if context is None:
                raise ValueError("context required")
            ctx = context.to(dev, torch.float32).reshape(B * N, -1).contiguous()
        g = None if pl is None or pl.guidance is None else self._guide_device(pl.guidance, node_mask, dev)
        return AttrDict(h=h, tabs=tabs, topo=topo, topo_loop=topo, tail=None, ctx=ctx, g=g, chain=None, B=B, N=N, dev=dev,
                        stream=_stream(dev))

    def _run(self, st, pl, z, k_lo, k_hi, noise, inpaint=None):
        """Transitions k_lo .. k_hi-1 of the plan `pl` (positions counted from the start of the chain) on z [B,N,D] in place; returns
        (z, chain - the sink of a recording plan, kept in `st` for the next piece - or None).  `noise` = (randn_x, randn_h, rows,
        seed, sample id base): injected rows, or None, None and the generator's key.  `inpaint` = (fixed u8 [B*N], known xh, R) or,
        for partial masks, (fixed_x u8 [B*N], known xh, R, fixed_h u8 [B*N*F]): the channel bytes are attached like the restraints.
        The plan's loop terms are attached to the topology for the time of the loop.  The one place that picks the loop:
        guided -> hd_sample_path_guided; a path -> hd_sample_path(_inpaint); else the every-step hd_sample_loop(_inpaint), whose
        steps count down from T."""
        lib, topo = _lib.load(), st.topo_loop
        rx, rh, rows, seed, base = noise
        fixed, known, R, parts = (tuple(inpaint) + (None,))[:4] if inpaint is not None else (None, None, 0, None)
        zz = z if st.tail is None else torch.cat([z, st.tail], dim=1).contiguous()      # a pocket's fixed rows ride along
        mol = -1 if st.tail is None else st.N
        common = (_ptr(rx), _ptr(rh), rows, seed, base, int(self.use_graph))
        steer, dvs, crs, ran = getattr(pl, "steer", None), getattr(pl, "diversity", None), getattr(pl, "corrector", None), False
        # every term the plan asks for is closed behind the loop - also when its opening, the loop or another close raises
        with contextlib.ExitStack() as closes:
            if pl.restraints is not None:
                closes.callback(pl.restraints.rs.detach, topo)
                self._restrain_open(st.h, topo, st.tabs, pl.restraints, st.B, st.dev)
            if steer is not None:
                closes.callback(lambda: steering_mod.close(self, topo, steer, st.B, st.dev, st.stream, ran))
                self._steer_open(st.h, topo, st.tabs, steer, int(k_lo) == 0, st.dev)
            if dvs is not None:
                closes.callback(lambda: _lib.check(lib.hd_diversity_detach(topo.ptr), "hd_diversity_detach"))
                self._diversity_open(st.h, topo, st.tabs, dvs, st.dev)
            if crs is not None:
                closes.callback(lambda: _lib.check(lib.hd_corrector_detach(topo.ptr), "hd_corrector_detach"))
                self._corrector_open(st.h, topo, st.tabs, crs, st.dev)
            if pl.frames is not None:
                closes.callback(lambda: _lib.check(lib.hd_chain_detach(topo.ptr), "hd_chain_detach"))
                st.chain = self._chain_open(st.h, topo, st.tabs, pl.frames, pl.record, st.B, st.N, st.dev, st.chain)
            if parts is not None:
                closes.callback(lambda: _lib.check(lib.hd_inpaint_parts(st.h, topo.ptr, None, st.stream), "hd_inpaint_parts"))
                _lib.check(lib.hd_inpaint_parts(st.h, topo.ptr, parts.data_ptr(), st.stream), "hd_inpaint_parts")
            if st.g is not None:
                _lib.check(lib.hd_sample_path_guided(st.h, topo.ptr, zz.data_ptr(), st.ctx.data_ptr(), st.g.ctx_u.data_ptr(),
                                                     st.g.w.data_ptr(), st.g.rows, st.g.phi, int(k_lo), int(k_hi), *common,
                                                     _ptr(fixed), _ptr(known), int(R), st.stream), "hd_sample_path_guided")
            elif inpaint is not None:
                fn, name, lo, hi = (lib.hd_sample_path_inpaint, "hd_sample_path_inpaint", k_lo, k_hi) if pl.path is not None else \
                    (lib.hd_sample_loop_inpaint, "hd_sample_loop_inpaint", pl.K - k_lo, pl.K - k_hi)
                _lib.check(fn(st.h, topo.ptr, zz.data_ptr(), _ptr(st.ctx), -1, int(lo), int(hi), *common, fixed.data_ptr(),
                              known.data_ptr(), int(R), st.stream), name)
            else:
                fn, name, lo, hi = (lib.hd_sample_path, "hd_sample_path", k_lo, k_hi) if pl.path is not None else \
                    (lib.hd_sample_loop, "hd_sample_loop", pl.K - k_lo, pl.K - k_hi)
                _lib.check(fn(st.h, topo.ptr, zz.data_ptr(), _ptr(st.ctx), mol, int(lo), int(hi), *common, st.stream), name)
            ran = True
            if crs is not None and int(k_hi) > int(k_lo):
                self.corrector_last = corrector_mod.read_gains(topo, crs, st.B, st.dev, st.stream)
        return (zz if st.tail is None else zz[:, :st.N].contiguous()), st.chain

    def _decode(self, st, z, node_mask, edge_mask, fix_noise, noise, chain=None, inpaint=None, eps=None):
        """(x, h) of z_0 - and `chain` with cat(x, h) as its frame 0 - : the network call at t = 0 (guided as the loop's are; `eps`:
        the caller has made it) and the final decode.  `noise`: the sample id base (the generator's draw T + 1) or an injected
        (randn_x, randn_h) pair, None = torch.randn.  `inpaint` = (fixed u8, x_known, h_known): the known rows are put back; with a
        fourth element (fixed_h u8 [B*N*F]) the first is the position mask and the known parts are."""
        if eps is None:
            eps = self._decode_eps(st.topo, z, st.ctx, st.g)
        philox = (int(noise), self.T + 1) if isinstance(noise, (int, np.integer)) else None
        x, h = self._final_decode(z, eps, node_mask, edge_mask, st.tabs["decode"].numpy(), fix_noise, None if philox else noise,
                                  philox=philox)
        if inpaint is not None:
            x, h = x.contiguous(), h.contiguous()
            if len(inpaint) > 3 and inpaint[3] is not None:
                _lib.check(_lib.load().hd_inpaint_decode_fix_parts(st.h, st.topo.ptr, inpaint[0].data_ptr(), inpaint[3].data_ptr(),
                                                                   inpaint[1].data_ptr(), inpaint[2].data_ptr(), x.data_ptr(),
                                                                   h.data_ptr(), st.stream), "hd_inpaint_decode_fix_parts")
            else:
                _lib.check(_lib.load().hd_inpaint_decode_fix(st.h, st.topo.ptr, inpaint[0].data_ptr(), inpaint[1].data_ptr(),
                                                             inpaint[2].data_ptr(), x.data_ptr(), h.data_ptr(), st.stream),
                           "hd_inpaint_decode_fix")
        if chain is None:
            return x, h
        chain[0] = torch.cat([x, h], dim=2)
        return x, h, chain

    # ------------------------------------------------------------------ full reverse process
    @torch.no_grad()
    def sample_from_masks(self, node_mask: torch.Tensor, edge_mask: Optional[torch.Tensor], context=None,
                          fix_noise: bool = False, raw_noises: Optional[Sequence[Tuple[torch.Tensor, torch.Tensor]]] = None,
                          sample_id_base: int = 0, z_init: Optional[torch.Tensor] = None, pocket=None, *,
                          steps: Optional[int] = None, eta: Optional[float] = None, spacing: Optional[str] = None,
                          timesteps: Optional[Sequence[int]] = None, guidance_scale=None, guidance_context=None, guidance_rescale: Optional[float] = None,
                          solver: Optional[str] = None, lower_order_final: Optional[bool] = None,
                          keep_frames: Optional[int] = None, record: Optional[str] = None,
                          restraints=None, restraint_scale=None, restraint_schedule=None, restraint_clip=None,
                          particles=None, steer_scale=None, steer_ess=None, steer_schedule=None, restraint_frame=None, diversity=None, corrector=None):
        """z_T -> (x, h) for given masks: draw z_T, T posterior steps, final decode.

        restraints / restraint_scale / restraint_schedule / restraint_clip (keyword-only; None: the model's attributes of the same
        names): restraint-guided sampling (hierdiff_amd/restraints.py) - at every transition of the chain the gradient of an energy
        U (obstacles, pair distances, anchors; a `restraints.Restraints`) on the network's data prediction goes into eps^, scaled by
        `restraint_scale` (a float or a [B] tensor) times the schedule's lambda_k ("score": nv0 sigma_t / alpha_t, "sigma": sigma_t,
        or K explicit weights), clipped per node to `restraint_clip` and freed of its mean, inside the library's loop (the identity
        path when no few-step path is asked for).  Coordinates are in data units in the MODEL'S frame: the centre of mass of the
        molecule's valid nodes is the origin, so obstacles and anchors are placed relative to where the molecule's centre sits.  The
        final decode at t = 0 is the network's own.  No restraints, or a scale of None or 0, is the unrestrained code path,
        untouched.  Combines with steps / eta / spacing / timesteps, solver "dpm2m", guidance and keep_frames.  Not with pocket
        models, mode 'gnn_dynamics' or noise_mode 'torch'.  Mechanism only: which scale, schedule and clip help is for the user to
        validate on a trained checkpoint.

        particles / steer_scale / steer_ess / steer_schedule (keyword-only; None: the model's `particles` / `steer_scale` /
        `steer_ess`): steered sampling (hierdiff_amd/steering.py) - the batch is G groups of `particles` rows (group g owns rows
        g P .. g P + P - 1, which must have equal masks, contexts and restraint rows); at every transition the rows of a group are
        weighted by the change of the restraint energy of their data prediction, logw += -steer_scale (U_k - U_prev) (times the k-th
        value of `steer_schedule`), and resampled systematically inside the library's loop when their effective sample size falls below
        steer_ess * P (default 0.5).  Needs `restraints`; `restraint_scale` may be None or 0 (selection without the gradient
        update).  The state of the call is left as `self.steer_last` (`steering.Result`).  A group's result depends on the seed, the
        ids of its rows, P and its own masks and tables only.  particles of None or 1, or a steer_scale of None or 0, is the unsteered
        code path, untouched.  Not with eta = 0, solver "dpm2m" (solver "sde2m" is the second-order update that steers), fix_noise, raw_noises, pocket models, mode 'gnn_dynamics' or
        noise_mode 'torch'.  Mechanism only.

        diversity (keyword-only; None: the model's `diversity`): a `diversity.Diversity(particles=P, length=l, strength=kappa, scale,
        schedule, clip)` - diverse sampling (hierdiff_amd/diversity.py).  The batch is G groups of P rows with equal masks and contexts;
        at every transition, behind guidance and the restraint updates, the rows of a group repel each other through
        Phi = kappa sum_{p<q} exp(-d2_pq / (2 l^2)) of the aligned RMSD d_pq of their data predictions, fed into eps^ like a restraint
        gradient (hd_diversity_attach, k_diverse_eps).  A gradient, not a selection: it also acts with eta = 0 and solver "dpm2m", and
        needs no restraints.  `self.diversity_last` (`diversity.Result`) holds Phi and the pairwise RMSD of the returned x.  None,
        particles = 1, or a strength or scale of 0 is the code path without it, untouched.  Not together with particles= (steering),
        fix_noise on a path that draws, pocket models, mode 'gnn_dynamics' or noise_mode 'torch'.  Mechanism only.

        keep_frames / record (keyword-only; None: nothing is recorded and the call is today's): the reference's `sample_chain`
        (en_diffusion.py:669-710) - the chain runs in the path loop (the identity path when no few-step path is asked for) with a
        sink attached, and a third tensor comes back: chain [keep_frames, B, N, D] on the device, in data units (`unnormalize`).
        Frame (p * keep_frames) // K holds the state at path position p counted from the t = 0 end (`paths.chain_frames`: the last
        state that falls into a frame stays, as in the reference), frame 0 is cat(x, h) of the decode.  record="x0" keeps the data
        prediction of the same transitions instead of their states.  1 <= keep_frames <= K.  (x, h) are the bits of the same call
        without recording.  Not with pocket models, mode 'gnn_dynamics' or noise_mode 'torch'.

        solver / lower_order_final (keyword-only; None: the model's `sample_solver` / `sample_lower_order_final`): None and "ddim" are the first-order
        updates below; "dpm2m" runs the path with DPM-Solver++(2M) (hd_set_path_multistep: the eta = 0 update plus a correction
        from the previous transition's data prediction, kept in a topology-owned buffer; second order, no extra network call,
        first order on the first and - with lower_order_final - the last transition).  It is deterministic on the path: `eta`
        defaults to 0 whatever `sample_eta` says, another explicit eta raises ValueError; steps / spacing / timesteps / guidance_*
        combine as usual, and the draws are z_T (draw 0) and the decode (T + 1) alone.  "sde2m" runs SDE-DPM-Solver++(2M)
        (hd_set_path_multistep_sde): the same correction, with c2 = alpha_s (-expm1(-2 h)) / (2 r), on the ancestral update - second
        order with the ancestral noise on the path, so it combines with steering (particles=); `eta` defaults to 1 whatever
        `sample_eta` says, another explicit eta raises ValueError; draws and `raw_noises` (K + 2 pairs) are those of eta = 1 on
        the same path, and fix_noise works.  Mechanism only, as `steps` / `eta`.

        guidance_scale / guidance_context / guidance_rescale (keyword-only; None: the model's attributes of the same names):
        classifier-free guidance of a context-conditioned model - every network call of the chain (the decode's included) runs
        under `context` and under `guidance_context` ([B,N,C]; None: the model's `null_context`) and eps_u + w (eps_c - eps_u) goes
        into the unchanged update, inside the library's loop (hd_sample_path_guided; the identity path when no few-step path is
        asked for).  `guidance_scale`: a float or a [B] tensor (per molecule); `guidance_rescale` phi in [0, 1] rescales the
        combination towards the spread of eps_c.  None, or a scalar 1.0 without a guidance_context, is the unguided code path,
        untouched.  Draws are those of the unguided chain.  Mechanism only: the model must have been trained with context dropout
        (`context_drop_prob`), and which scale helps is for the user to validate on a trained checkpoint.

        steps / eta / spacing / timesteps (keyword-only; None: the model's `sample_steps` / `sample_eta` / `sample_spacing` /
        `sample_timesteps`): few-step sampling - K = steps transitions on a sub-sequence of the trained grid ("uniform" or
        "quadratic" spacing, or the explicit decreasing list `timesteps` from T to 0), ancestral (eta = 1) or with the DDIM-family
        update (0 <= eta < 1; eta = 0 draws no noise on the path), inside the library's loop (hd_sample_path).  Noise counters are
        those of the visited fine-grid steps, so a sample still depends only on its global id; `raw_noises` then holds K + 2
        pairs (z_T, the K transitions, decode).  The defaults run today's full chain through the plain loop.  The mechanism is
        exact; which K and eta keep sample quality is for the user to validate on a trained checkpoint.

        raw_noises: optional T+2 (randn_x[b,N,3], randn_h[b,N,F]) pairs in the reference's draw order
        (z_T, steps s=T-1..0, decode) for bit-for-bit comparable trajectories; otherwise noise comes
        from `noise_mode` ("philox": sample ids sample_id_base + b, independent of batch split).
        pocket: optional (pos [B,P,3], feat [B,P,F] already embedded, node_mask [B,P,1], edge_mask [B,P,P]) of fixed
        residue nodes: appended to z for every network call with a block-diagonal edge mask and never updated
        (diffusion_qm9.py:362-371,381-382); the final decode sees the molecule alone (:386-387)."""
        dev = node_mask.device
        B, N = int(node_mask.shape[0]), int(node_mask.shape[1])
        pl = self._plan("sample_from_masks", pocket=pocket, injected=raw_noises is not None, B=B, N=N, fix_noise=fix_noise, **given(locals()))
        if pl.guidance is not None and context is None:
            raise ValueError("context required")
        gnn = getattr(self.dynamics, "mode", "egnn_dynamics") == "gnn_dynamics"
        if pl.path is not None and (gnn or (self.noise_mode == "torch" and raw_noises is None)):
            raise NotImplementedError("few-step sampling runs inside the library's loop: mode 'gnn_dynamics' and noise_mode 'torch' "
                                      "(step-by-step Python loops) take the full chain only")
        st = self._device_state(node_mask, edge_mask, context, B, N, pl)
        lib, h, topo, stream, K, T = _lib.load(), st.h, st.topo, st.stream, pl.K, self.T
        if pocket is not None:
            if st.ctx is not None or self.noise_mode == "torch":
                raise NotImplementedError("pocket conditioning: context=None and library/injected noise only")
            p_pos, p_feat, p_nm, p_em = pocket
            P = p_pos.shape[1]
            st.tail = torch.cat([p_pos.to(dev, torch.float32), p_feat.to(dev, torch.float32)], dim=-1)
            nmb = node_mask.to(torch.bool)
            em_mol = edge_mask.to(torch.bool).reshape(B, N, N) if edge_mask is not None else \
                (nmb & nmb.transpose(1, 2) & ~torch.eye(N, dtype=torch.bool, device=dev)[None])
            self._nm_cat = torch.cat([nmb, p_nm.to(dev).bool()], dim=1)
            self._em_cat = torch.zeros(B, N + P, N + P, dtype=torch.bool, device=dev)
            self._em_cat[:, :N, :N] = em_mol
            self._em_cat[:, N:, N:] = p_em.to(dev).bool()
            st.topo_loop = self.dynamics.topology(self._nm_cat, self._em_cat, B, N + P)
        nb = 1 if fix_noise else B
        z = torch.empty((B, N, self.n_dims + self.in_node_nf), device=dev, dtype=torch.float32)
        chain = None
        if gnn and (pocket is not None or z_init is not None):
            raise NotImplementedError("mode 'gnn_dynamics': plain sampling only (no pocket, no z_init)")
        if gnn and raw_noises is not None:
            # step by step (the fused loop evaluates the egnn network): injected draws in the reference's order
            assert len(raw_noises) == T + 2, "need T+2 raw noise pairs"
            z = self._combine_raw(raw_noises[0], node_mask, B)
            gg = None if self.schedule_gammas is None else torch.as_tensor(np.asarray(self.schedule_gammas), dtype=torch.float32)
            for i, s_ in enumerate(reversed(range(0, T))):
                s_array = torch.full((B, 1), fill_value=s_, device=dev)
                gm = None if gg is None else (gg[s_].expand(B, 1), gg[s_ + 1].expand(B, 1))
                z = self.sample_p_zs_given_zt(s_array / T, (s_array + 1) / T, z, node_mask, edge_mask, context, fix_noise=fix_noise,
                                              mol_shape=N, raw_noise=raw_noises[1 + i], gammas=gm)
            final = tuple(r.to(dev, torch.float32).contiguous() for r in raw_noises[T + 1])
        elif raw_noises is not None:
            assert len(raw_noises) == K + 2, "need T+2 raw noise pairs (few-step sampling: steps + 2)"
            rx = [r[0].to(dev, torch.float32).contiguous() for r in raw_noises]
            rh = [r[1].to(dev, torch.float32).contiguous() for r in raw_noises]
            _lib.check(lib.hd_noise(h, topo.ptr, rx[0].data_ptr(), rh[0].data_ptr(), rx[0].shape[0], 0, 0, 0, 0,
                                    z.data_ptr(), stream), "hd_noise")
            step_x = torch.stack(rx[1:K + 1]).contiguous()
            step_h = torch.stack(rh[1:K + 1]).contiguous()
            z, chain = self._run(st, pl, z, 0, K, (step_x, step_h, step_x.shape[1], 0, 0))
            final = (rx[K + 1], rh[K + 1])
        elif self.noise_mode == "torch" or gnn:
            z = self.sample_combined_position_feature_noise(nb, N, node_mask)
            if nb == 1 and B > 1:
                z = z.expand(B, -1, -1).contiguous()
            for s in reversed(range(0, T)):
                s_array = torch.full((B, 1), fill_value=s, device=dev)
                z = self.sample_p_zs_given_zt(s_array / T, (s_array + 1) / T, z, node_mask, edge_mask, context,
                                              fix_noise=fix_noise, mol_shape=N)
            final = None                                 # torch.randn draws
        else:
            if z_init is not None:
                z.copy_(z_init)
            else:
                _lib.check(lib.hd_noise(h, topo.ptr, None, None, nb, self.seed, sample_id_base, 0, int(fix_noise),
                                        z.data_ptr(), stream), "hd_noise")
            z, chain = self._run(st, pl, z, 0, K, (None, None, nb, self.seed, sample_id_base))
            final = int(sample_id_base)                  # decode noise: draw T+1 of the same counter stream
        self._check_mean_zero(z[:, :, :self.n_dims], node_mask)
        eps = self.phi(z, torch.zeros((B, 1), device=dev), node_mask, edge_mask, context) if gnn else None
        out = self._decode(st, z, node_mask, edge_mask, fix_noise, final, chain, eps=eps)
        self._diversity_result(pl, out[0], node_mask)
        return out

    @torch.no_grad()
    def path_steps(self, z, node_mask, edge_mask=None, context=None, *, steps=None, eta=None, spacing=None, timesteps=None,
                   k_lo: int = 0, k_hi: Optional[int] = None, sample_id_base: int = 0, fix_noise: bool = False,
                   guidance_scale=None, guidance_context=None, guidance_rescale: Optional[float] = None,
                   solver: Optional[str] = None, lower_order_final: Optional[bool] = None,
                   restraints=None, restraint_scale=None, restraint_schedule=None, restraint_clip=None,
                   particles=None, steer_scale=None, steer_ess=None, steer_schedule=None, restraint_frame=None, diversity=None, corrector=None):
        """Transitions k_lo .. k_hi-1 of `sample_from_masks`'s few-step loop on a given z [B,N,D] (normalised units, the state at
        path position k_lo); returns the state at position k_hi (default: the end of the path, z_0 before the decode).  Draws are
        keyed by the arrival step, so a chain cut into pieces gives the bits of the whole.
        solver="dpm2m" / "sde2m": transition k > 0 also needs the data prediction of transition k - 1, which the library keeps with the
        topology (the masks).  A call with k_lo > 0 must therefore continue the previous call on the same masks and the same path
        exactly where that call ended (its k_hi); a piece-wise chain then gives the bits of the whole.  Anything else - fresh masks,
        another path or solver in between, a gap - raises HierDiffHipError (HD_E_STATE) instead of using a stale prediction."""
        B, N = int(node_mask.shape[0]), int(node_mask.shape[1])
        pl = self._plan("path_steps", force_path=True, B=B, N=N, fix_noise=fix_noise, **given(locals()))       # also the identity path goes through hd_sample_path here
        if getattr(self.dynamics, "mode", "egnn_dynamics") == "gnn_dynamics" or self.noise_mode == "torch":
            raise NotImplementedError("few-step sampling: mode 'gnn_dynamics' and noise_mode 'torch' are not supported")
        k_hi = pl.K if k_hi is None else int(k_hi)
        if tuple(z.shape) != (B, N, self.n_dims + self.in_node_nf) or not (0 <= int(k_lo) <= k_hi <= pl.K):
            raise ValueError("z must be [B, N, 3 + F] and 0 <= k_lo <= k_hi <= steps")
        if pl.guidance is not None and context is None:
            raise ValueError("context required")
        st = self._device_state(node_mask, edge_mask, context, B, N, pl)
        z = z.detach().to(st.dev, torch.float32).clone().contiguous()
        return self._run(st, pl, z, k_lo, k_hi, (None, None, 1 if fix_noise else B, self.seed, sample_id_base))[0]

    # ------------------------------------------------------------------ scoring: every term of the bound (no reference counterpart)
    def _nll_tables(self, handle, tabs, t_list):
        """Rows of the terms from the gamma grid of `_schedule`, uploaded to the handle (hd_set_nll_terms) once per (table, list)."""
        from . import scoring
        key = tuple(t_list)
        hit = self.__dict__.get("_nll_cache")
        if hit is None or hit[0] is not tabs or hit[1] != key:
            tt = scoring.term_tables(tabs["gamma"], t_list)
            t_idx = np.ascontiguousarray(tt["t_idx"].numpy(), dtype=np.int32)
            coef = np.ascontiguousarray(tt["coef"].numpy(), dtype=np.float32)
            self._nll_cache = None
            _lib.check(_lib.load().hd_set_nll_terms(handle, tt["K"], t_idx.ctypes.data_as(C.POINTER(C.c_int)),
                                                    coef.ctypes.data_as(C.POINTER(C.c_float))), "hd_set_nll_terms")
            self._nll_cache = (tabs, key, tt)
        return self._nll_cache[2]

    def _nll_setup(self, x, h, node_mask, edge_mask, context, terms, timesteps, seed, sample_id_base, raw_noises, return_terms,
                   use_graph):
        """Argument checks of `nll_full` (ValueError / NotImplementedError before anything is queued), then the device-side inputs of
        hd_nll_terms / hd_nll_finish."""
        from . import scoring
        t_list = scoring.resolve_terms(self.T, terms, timesteps)
        K = len(t_list)
        if self.pocket:
            raise ValueError("nll_full: pocket models / mol_shape are not supported (the score covers whole molecules)")
        if node_mask.dim() != 3 or node_mask.shape[2] != 1:
            raise ValueError(f"node_mask must be [B, N, 1], got {tuple(node_mask.shape)}")
        B, N = int(node_mask.shape[0]), int(node_mask.shape[1])
        F_ = self.in_node_nf
        if tuple(x.shape) != (B, N, self.n_dims):
            raise ValueError(f"x must be [{B}, {N}, {self.n_dims}], got {tuple(x.shape)}")
        if tuple(h.shape) != (B, N, F_):
            raise ValueError(f"h must be [{B}, {N}, {F_}], got {tuple(h.shape)}")
        if edge_mask is not None and edge_mask.numel() != B * N * N:
            raise ValueError(f"edge_mask must hold {B} x {N} x {N} entries")
        if self.dynamics.context_node_nf > 0 and context is None:
            raise ValueError("context required")
        if raw_noises is not None:
            if len(raw_noises) != K + 1:
                raise ValueError(f"raw_noises must hold {K} + 1 (randn_x, randn_h) pairs: one per term in list order, then eps_0")
            for rx_, rh_ in raw_noises:
                if tuple(rx_.shape) != (B, N, self.n_dims) or tuple(rh_.shape) != (B, N, F_):
                    raise ValueError(f"raw_noises pairs must be ([{B}, {N}, {self.n_dims}], [{B}, {N}, {F_}])")
        if isinstance(sample_id_base, bool) or int(sample_id_base) != sample_id_base or int(sample_id_base) < 0:
            raise ValueError(f"sample_id_base must be an integer >= 0, got {sample_id_base!r}")
        if getattr(self.dynamics, "mode", "egnn_dynamics") == "gnn_dynamics":
            raise NotImplementedError("nll_full: mode 'gnn_dynamics' is not supported")
        dev = x.device
        if dev.type != "cuda":
            raise _lib.HierDiffHipError("scoring runs only on an MI355X (no CPU fallback)")
        handle = self._lib_handle()
        tabs = self._schedule(rows=B)
        self._nll_tables(handle, tabs, t_list)
        node_mask = node_mask.to(dev)
        topo = self.dynamics.topology(node_mask, edge_mask, B, N)
        ctx = None
        if self.dynamics.context_node_nf > 0:
            ctx = context.to(dev, torch.float32).reshape(B * N, -1).contiguous()
        x_n, h_n, _ = self.normalize(x.to(torch.float32), h.to(dev, torch.float32), node_mask.to(torch.float32))
        xh = torch.cat([x_n, h_n], dim=2).contiguous()
        rx = rh = None
        if raw_noises is not None:
            rx = torch.stack([r[0].to(dev, torch.float32) for r in raw_noises]).contiguous()
            rh = torch.stack([r[1].to(dev, torch.float32) for r in raw_noises]).contiguous()
        g = tabs["gamma"].to(torch.float32).reshape(-1)
        consts = np.array([float(torch.sqrt(torch.sigmoid(-g[0]))), float(torch.sqrt(torch.sigmoid(g[0]))), float(g[0]),
                           float(g[self.T]), float(self.norm_values[2]), float(self.norm_biases[2] or 0.0),
                           math.log(float(self.norm_values[0]))], dtype=np.float32)
        return AttrDict(h=handle, topo=topo, ctx=ctx, xh=xh, rx=rx, rh=rh, B=B, N=N, K=K, t_list=t_list, consts=consts,
                        seed=int(self.seed if seed is None else seed), base=int(sample_id_base), use_graph=int(bool(use_graph)),
                        acc=torch.zeros(B, dtype=torch.float64, device=dev),
                        err=torch.zeros((K, B), dtype=torch.float32, device=dev) if return_terms else None,
                        stream=_stream(dev), dev=dev)

    def _nll_terms(self, st, k_lo: int, k_hi: int):
        """Terms k_lo .. k_hi-1 of the list into st.acc (and st.err)."""
        nd, F_ = self.n_dims, self.in_node_nf
        per = st.B * st.N
        _lib.check(_lib.load().hd_nll_terms(
            st.h, st.topo.ptr, st.xh.data_ptr(), _ptr(st.ctx), -1, int(k_lo), int(k_hi),
            None if st.rx is None else st.rx.data_ptr() + 4 * per * nd * int(k_lo),
            None if st.rh is None else st.rh.data_ptr() + 4 * per * F_ * int(k_lo), st.B, st.seed, st.base, st.use_graph,
            st.acc.data_ptr(), _ptr(st.err), st.stream), "hd_nll_terms")

    def _nll_finish(self, st):
        int_nf, cont_nf = (5, 3) if self.node_coarse_type == 'prop' else (3, 0)
        nd, F_ = self.n_dims, self.in_node_nf
        per = st.B * st.N
        nll = torch.empty(st.B, dtype=torch.float32, device=st.dev)
        _lib.check(_lib.load().hd_nll_finish(
            st.h, st.topo.ptr, st.xh.data_ptr(), _ptr(st.ctx), -1,
            None if st.rx is None else st.rx.data_ptr() + 4 * per * nd * st.K,
            None if st.rh is None else st.rh.data_ptr() + 4 * per * F_ * st.K, st.B, st.seed, st.base, st.K,
            st.consts.ctypes.data_as(C.POINTER(C.c_float)), int_nf, cont_nf, st.acc.data_ptr(), nll.data_ptr(), st.stream),
            "hd_nll_finish")
        return nll

    @torch.no_grad()
    def nll_full(self, x, h, node_mask, edge_mask=None, context=None, *, terms: Optional[int] = None,
                 timesteps: Optional[Sequence[int]] = None, seed: Optional[int] = None, sample_id_base: int = 0,
                 raw_noises: Optional[Sequence[Tuple[torch.Tensor, torch.Tensor]]] = None, return_terms: bool = False,
                 use_graph: bool = True):
        """nll [B] of raw data (x, h) in the units of eval-mode `nll`, with EVERY term of the variational bound evaluated instead of
        one random t:  kl_prior + (T / K) sum_{t in S} L_t + neg_log_constants + L_0 - delta_log_px,  L_t = 0.5 (SNR(g_s - g_t) - 1)
        |eps_t - eps^_t|^2 - inside the library's loop (hd_nll_terms: one captured term per topology, replayed K times; algorithm and
        draw layout in include/hierdiff_hip.h).  S = all of 1 .. T (default: exact in t, still one noise draw per term), the K
        visited steps of a uniform K-step path (`terms=K`, stratified with the factor T / K) or an explicit subset (`timesteps`).
        Noise: the counter-based generator at (seed or `self.seed`, sample_id_base + row, draw = t; eps_0: draw 0), so a molecule's
        score depends on its global id, its mask, the weights, the schedule and its data only; `raw_noises` instead injects K + 1
        (randn_x [B,N,3], randn_h [B,N,F]) pairs - the terms in list order (descending t), then eps_0.  With `return_terms` also
        (t_idx [K], e_t [K, B]), the `error` of the reference's info dict per term.  Independent of `self.training`; no gradients
        (training keeps the one-t estimator).  Pocket models raise ValueError.  Scores of untrained weights mean nothing
        chemically."""
        st = self._nll_setup(x, h, node_mask, edge_mask, context, terms, timesteps, seed, sample_id_base, raw_noises, return_terms,
                             use_graph)
        self._nll_terms(st, 0, st.K)
        nll = self._nll_finish(st)
        if return_terms:
            return nll, (torch.tensor(st.t_list, dtype=torch.int64), st.err)
        return nll

    @torch.no_grad()
    def score(self, samples: Sequence[Dict[str, torch.Tensor]], device, batch_size: int = 256, **kw):
        """`nll_full` for a list in the sampler's result format [{'x': [n,3], 'h': [n,F] (, 'context')}] (what `sample` returns and
        stage 2 consumes): padded to batches of `batch_size`, x re-centred per molecule, molecule i scored under the sample id
        sample_id_base + i.  Returns a CPU tensor [len(samples)].  Keywords: terms / timesteps / seed / sample_id_base / use_graph
        of `nll_full`."""
        from . import scoring
        device = torch.device(device)
        corrector_mod.refuse(self, "score", kw.get("corrector"), ": it evaluates the bound of given molecules and samples nothing")
        extra = set(kw) - {"terms", "timesteps", "seed", "sample_id_base", "use_graph"}
        if extra:
            raise ValueError(f"score: unsupported keyword(s) {sorted(extra)} (terms, timesteps, seed, sample_id_base, use_graph)")
        base = kw.pop("sample_id_base", 0)
        scoring.resolve_terms(self.T, kw.get("terms"), kw.get("timesteps"))          # argument errors first
        if isinstance(batch_size, bool) or int(batch_size) != batch_size or int(batch_size) < 1:
            raise ValueError(f"batch_size must be an integer >= 1, got {batch_size!r}")
        samples = list(samples)
        if not samples:
            raise ValueError("score: no samples")
        with_ctx = self.dynamics.context_node_nf > 0
        batches = [scoring.pad_samples(samples[lo:lo + int(batch_size)], self.n_dims, self.in_node_nf, with_ctx)
                   for lo in range(0, len(samples), int(batch_size))]
        out = []
        for i, (x, h, nm, ctx) in enumerate(batches):
            out.append(self.nll_full(x.to(device), h.to(device), nm.to(device), None, None if ctx is None else ctx.to(device),
                                     sample_id_base=base + i * int(batch_size), **kw).cpu())
        return torch.cat(out)

    # ------------------------------------------------------------------ editing given molecules (no reference counterpart)
    def _up_tables(self, handle, tabs, path):
        """Rows of the ascending `path` from the gamma grid of `_schedule`, uploaded to the handle (hd_set_path_up): the tables that
        hd_set_path fills, so the two directions share one cache (`_upload_path`)."""
        from . import paths
        ip = lambda a: np.ascontiguousarray(a.numpy(), dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int))

        def upload(ut):
            coef = np.ascontiguousarray(ut["coef"].numpy(), dtype=np.float32)
            _lib.check(_lib.load().hd_set_path_up(handle, ut["K"], ip(ut["from_idx"]), ip(ut["to_idx"]),
                                                  coef.ctypes.data_as(C.POINTER(C.c_float))), "hd_set_path_up")

        return self._upload_path(tabs, (tuple(path), "up"), lambda: paths.up_tables(tabs["gamma"], path), upload)

    def _grid_index(self, t, lo: int, what: str) -> int:
        if isinstance(t, torch.Tensor) and t.numel() == 1 and not t.is_floating_point():
            t = int(t)
        if isinstance(t, bool) or not isinstance(t, (int, np.integer)) or not (lo <= int(t) <= self.T):
            raise ValueError(f"{what} must be a grid index in {lo} .. {self.T}, got {t!r}")
        return int(t)

    def _edit_check(self, what: str, node_mask, z_shapes=(), context=None, sample_id_base=0, needs_noise: bool = False,
                    needs_context: bool = True):
        """Argument and configuration errors of the editing entry points, all raised before the GPU is touched."""
        if not isinstance(node_mask, torch.Tensor) or node_mask.dim() != 3 or node_mask.shape[2] != 1:
            raise ValueError(f"node_mask must be [B, N, 1], got {tuple(getattr(node_mask, 'shape', ()))}")
        B, N = int(node_mask.shape[0]), int(node_mask.shape[1])
        for name, t, width in z_shapes:
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != (B, N, width):
                raise ValueError(f"{name} must be [{B}, {N}, {width}], got {tuple(getattr(t, 'shape', ()))}")
        if needs_context and self.dynamics.context_node_nf > 0 and context is None:
            raise ValueError("context required")
        if isinstance(sample_id_base, bool) or int(sample_id_base) != sample_id_base or int(sample_id_base) < 0:
            raise ValueError(f"sample_id_base must be an integer >= 0, got {sample_id_base!r}")
        unsupported(self, what, None, needs_noise, pocket_error=ValueError)
        return B, N

    def _edit_device(self, node_mask, edge_mask, context, B, N, pl=None):
        """`_device_state` of the editing entry points (`diffuse` and `slerp` call no network: no context)."""
        return self._device_state(node_mask, edge_mask, context, B, N, pl, what="editing", needs_context=False)

    def _alpha_sigma(self, tabs, t: int):
        """(alpha_t, sigma_t) as the loss and `scoring.term_tables` compute them: fp32 sqrt(sigmoid(-+gamma_t)) of the fp32 grid."""
        g = tabs["gamma"].to(torch.float32).reshape(-1)[t]
        return float(torch.sqrt(torch.sigmoid(-g))), float(torch.sqrt(torch.sigmoid(g)))

    def _diffuse_xh(self, st, x, h, node_mask, alpha, sigma, raw, nb, seed, base, share):
        """z = alpha xh + sigma eps through hd_diffuse: x re-centred per molecule, (x, h) normalised."""
        nmf = node_mask.to(st.dev, torch.float32)
        x = x.to(st.dev, torch.float32) * nmf
        x = x - (x.sum(1, keepdim=True) / nmf.sum(1, keepdim=True).clamp(min=1.0)) * nmf
        x_n, h_n, _ = self.normalize(x, h.to(st.dev, torch.float32), nmf)
        xh = torch.cat([x_n, h_n], dim=2).contiguous()
        z = torch.empty_like(xh)
        rx = rh = None
        if raw is not None:
            rx, rh = (r.to(st.dev, torch.float32).contiguous() for r in raw)
        _lib.check(_lib.load().hd_diffuse(st.h, st.topo.ptr, xh.data_ptr(), alpha, sigma, _ptr(rx), _ptr(rh), nb, seed, base, 0,
                                          share, z.data_ptr(), st.stream), "hd_diffuse")
        return z

    @torch.no_grad()
    def diffuse(self, x, h, node_mask, t, *, edge_mask=None, seed: Optional[int] = None, sample_id_base: int = 0,
                raw_noise: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, fix_noise: bool = False):
        """z_t [B,N,D] = alpha_t xh + sigma_t eps in normalised units for raw data (x [B,N,3], h [B,N,F]) at the grid index `t` in
        0 .. T: the start state of `sample_from_latent(t_start=t)` (variations of given molecules; hd_diffuse).  x is re-centred per
        molecule, as `score` does.  eps is the combined noise (masked, x part mean-free): the counter-based generator at (seed or
        `self.seed`, sample_id_base + row, draw 0) - the slot plain sampling uses for z_T, layout in include/hierdiff_hip.h - or the
        injected `raw_noise` = (randn_x [b,N,3], randn_h [b,N,F]), b = 1 with `fix_noise` (one row shared by the batch), else B."""
        F_ = self.in_node_nf
        t = self._grid_index(t, 0, "t")
        B, N = self._edit_check("diffuse", node_mask, (("x", x, self.n_dims), ("h", h, F_)), sample_id_base=sample_id_base,
                                needs_noise=raw_noise is None, needs_context=False)
        nb = 1 if fix_noise else B
        if raw_noise is not None and (tuple(raw_noise[0].shape) != (nb, N, self.n_dims) or tuple(raw_noise[1].shape) != (nb, N, F_)):
            raise ValueError(f"raw_noise must be ([{nb}, {N}, {self.n_dims}], [{nb}, {N}, {F_}])")
        st = self._edit_device(node_mask, edge_mask, None, B, N)
        alpha, sigma = self._alpha_sigma(st.tabs, t)
        return self._diffuse_xh(st, x, h, node_mask, alpha, sigma, raw_noise, nb, int(self.seed if seed is None else seed),
                                int(sample_id_base), int(fix_noise))

    @torch.no_grad()
    def encode(self, x, h, node_mask, edge_mask=None, context=None, *, t_end: Optional[int] = None, steps: Optional[int] = None,
               spacing: Optional[str] = None, timesteps: Optional[Sequence[int]] = None, solver: Optional[str] = None,
               restraints=None):
        """The latent z_{t_end} [B,N,D] (default t_end = T) of raw data (x, h): z_0 = alpha_0 xh without noise, then the deterministic
        eta = 0 update of the DDIM family run UPWARDS in t ("DDIM inversion") on `paths.ascending_path(T, t_end, steps, spacing,
        timesteps)` - default every grid point - inside the library's loop (hd_set_path_up / hd_sample_path: one captured transition
        per topology).  Nothing is drawn: the result depends on the data, the masks, the weights and the path only.  Decoding with
        `sample_from_latent(eta=0)` on the same points comes back near the molecule; how near is a property of the weights and K.
        The inversion stays first order: solver="dpm2m" or "sde2m" raises ValueError (the model's `sample_solver` is not consulted)."""
        from . import paths, restraints as _rs
        _rs.refuse(self, "encode", restraints, ": the inversion follows the network's own flow")
        steering_mod.refuse(self, "encode")
        diversity_mod.refuse(self, "encode", None, ": the inversion follows the network's own flow")
        corrector_mod.refuse(self, "encode", None, ": the inversion follows the network's own flow")
        if paths.check_solver(solver) is not None:
            raise ValueError(f"encode: the inversion is first order (eta = 0 upwards); solver {solver!r} is not supported")
        t_end = self._grid_index(self.T if t_end is None else t_end, 1, "t_end")
        spacing = self.sample_spacing if spacing is None else spacing
        path = paths.ascending_path(self.T, t_end, steps, spacing, timesteps)
        B, N = self._edit_check("encode", node_mask, (("x", x, self.n_dims), ("h", h, self.in_node_nf)), context)
        st = self._edit_device(node_mask, edge_mask, context, B, N)
        alpha0, _ = self._alpha_sigma(st.tabs, 0)
        z = self._diffuse_xh(st, x, h, node_mask, alpha0, 0.0, None, B, 0, 0, 0)
        K = self._up_tables(st.h, st.tabs, path)["K"]
        _lib.check(_lib.load().hd_sample_path(st.h, st.topo.ptr, z.data_ptr(), _ptr(st.ctx), -1, 0, K, None, None, B, 0, 0,
                                              int(self.use_graph), st.stream), "hd_sample_path")
        return z

    def _latent_path(self, t_start, steps, eta, spacing, timesteps, solver=None, lower_order_final=None):
        """(t_start, partial path, eta - or the `paths.Multistep` of solver "dpm2m") of the keywords: a view of `plan.latent_path`."""
        return latent_path(self, t_start, steps, eta, spacing, timesteps, solver, lower_order_final)

    @staticmethod
    def _batch_of(node_mask):
        """(B, N) for the plan, where the mask already looks like one (its shape errors come after the plan's)."""
        ok = isinstance(node_mask, torch.Tensor) and node_mask.dim() == 3
        return (int(node_mask.shape[0]), int(node_mask.shape[1])) if ok else (None, None)

    def _latent_run(self, pl, z, node_mask, edge_mask, context, k_lo, k_hi, sample_id_base, fix_noise, raw_noises):
        """Shape checks, device state and the transitions k_lo .. k_hi-1 of a partial chain: (state, z at k_hi, chain or None)."""
        B, N = self._edit_check("sample_from_latent", node_mask, (("z", z, self.n_dims + self.in_node_nf),), context, sample_id_base,
                                needs_noise=raw_noises is None)
        nb = 1 if fix_noise else B
        if raw_noises is not None:
            if len(raw_noises) != k_hi - k_lo:
                raise ValueError(f"raw_noises must hold one (randn_x, randn_h) pair per transition ({k_hi - k_lo})")
            for rx_, rh_ in raw_noises:
                if tuple(rx_.shape) != (nb, N, self.n_dims) or tuple(rh_.shape) != (nb, N, self.in_node_nf):
                    raise ValueError(f"raw_noises pairs must be ([{nb}, {N}, {self.n_dims}], [{nb}, {N}, {self.in_node_nf}])")
        st = self._edit_device(node_mask, edge_mask, context, B, N, pl)
        z = z.detach().to(st.dev, torch.float32).clone().contiguous()
        noise = (None, None, nb, self.seed, int(sample_id_base))
        if raw_noises is not None and k_hi > k_lo:
            noise = (torch.stack([r[0].to(st.dev, torch.float32) for r in raw_noises]).contiguous(),
                     torch.stack([r[1].to(st.dev, torch.float32) for r in raw_noises]).contiguous(), nb, 0, 0)
        return (st,) + self._run(st, pl, z, k_lo, k_hi, noise)

    @torch.no_grad()
    def latent_steps(self, z, node_mask, edge_mask=None, context=None, *, t_start: Optional[int] = None, steps: Optional[int] = None,
                     eta: Optional[float] = None, spacing: Optional[str] = None, timesteps: Optional[Sequence[int]] = None,
                     k_lo: int = 0, k_hi: Optional[int] = None, sample_id_base: int = 0, fix_noise: bool = False,
                     raw_noises: Optional[Sequence[Tuple[torch.Tensor, torch.Tensor]]] = None, guidance_scale=None, guidance_context=None, guidance_rescale: Optional[float] = None,
                     solver: Optional[str] = None, lower_order_final: Optional[bool] = None,
                     restraints=None, restraint_scale=None, restraint_schedule=None, restraint_clip=None,
                     particles=None, steer_scale=None, steer_ess=None, steer_schedule=None, restraint_frame=None, diversity=None, corrector=None):
        """Transitions k_lo .. k_hi-1 of `sample_from_latent`'s partial chain on a given z [B,N,D] (the state at path position k_lo);
        returns the state at position k_hi (default: the end, z_0 before the decode), as `path_steps` does for a full path.  Draws are
        keyed by the arrival step, so a chain cut into pieces gives the bits of the whole.  `raw_noises`: k_hi - k_lo injected
        (randn_x, randn_h) pairs, one per transition run.  solver="dpm2m" over a sub-range: the continuity rule of `path_steps`."""
        B, N = self._batch_of(node_mask)
        pl = self._plan("sample_from_latent", "latent", t_start=t_start, injected=raw_noises is not None, B=B, N=N, fix_noise=fix_noise,
                        **given(locals()))
        k_lo, k_hi = int(k_lo), pl.K if k_hi is None else int(k_hi)
        if not (0 <= k_lo <= k_hi <= pl.K):
            raise ValueError(f"need 0 <= k_lo <= k_hi <= {pl.K} (the path's transitions)")
        return self._latent_run(pl, z, node_mask, edge_mask, context, k_lo, k_hi, sample_id_base, fix_noise, raw_noises)[1]

    @torch.no_grad()
    def sample_from_latent(self, z, node_mask, edge_mask=None, context=None, *, t_start: Optional[int] = None,
                           steps: Optional[int] = None, eta: Optional[float] = None, spacing: Optional[str] = None,
                           timesteps: Optional[Sequence[int]] = None, sample_id_base: int = 0, fix_noise: bool = False,
                           raw_noises: Optional[Sequence[Tuple[torch.Tensor, torch.Tensor]]] = None, guidance_scale=None, guidance_context=None, guidance_rescale: Optional[float] = None,
                           solver: Optional[str] = None, lower_order_final: Optional[bool] = None,
                           keep_frames: Optional[int] = None, record: Optional[str] = None,
                           restraints=None, restraint_scale=None, restraint_schedule=None, restraint_clip=None,
                           particles=None, steer_scale=None, steer_ess=None, steer_schedule=None, restraint_frame=None, diversity=None, corrector=None):
        """(x, h) from a state z [B,N,D] at the grid index `t_start` (default T; normalised units - what `diffuse` and `encode`
        return): the partial reverse chain on `paths.partial_path(T, t_start, steps, spacing, timesteps)` (default: every grid point
        below t_start) inside the library's loop (hd_sample_path), then the final decode of `sample_from_masks`.  `eta` defaults to
        the model's `sample_eta`: 1 ancestral, 0 <= eta < 1 the DDIM family, 0 noise-free on the path.  Draws: T - s of the visited
        steps and T + 1 for the decode at (self.seed, sample_id_base + row) - plain sampling's layout, so t_start = T on the identity
        path is `sample_from_masks(z_init=z)` bit for bit; `raw_noises` instead injects K + 1 pairs (the K transitions, the decode).
        `t_start` sets how far variations drift from the lead; which t_start, K and eta are chemically useful is for the user to
        validate on a trained checkpoint.  solver / lower_order_final: as in `sample_from_masks` ("dpm2m": second order, eta = 0).
        keep_frames / record: as in `sample_from_masks` - a third tensor chain [keep_frames, B, N, D] of the partial chain.
        restraints / restraint_scale / restraint_schedule / restraint_clip: as in `sample_from_masks`, on the partial chain."""
        B, N = self._batch_of(node_mask)
        pl = self._plan("sample_from_latent", "latent", t_start=t_start, injected=raw_noises is not None, B=B, N=N, fix_noise=fix_noise,
                        **given(locals()))
        K = pl.K
        if raw_noises is not None and len(raw_noises) != K + 1:
            raise ValueError(f"raw_noises must hold {K} + 1 (randn_x, randn_h) pairs: the transitions, then the decode")
        st, z0, chain = self._latent_run(pl, z, node_mask, edge_mask, context, 0, K, sample_id_base, fix_noise,
                                         None if raw_noises is None else raw_noises[:K])
        node_mask = node_mask.to(st.dev)
        self._check_mean_zero(z0[:, :, :self.n_dims], node_mask)
        out = self._decode(st, z0, node_mask, edge_mask, fix_noise, int(sample_id_base) if raw_noises is None else raw_noises[K], chain)
        self._diversity_result(pl, out[0], node_mask)
        return out

    @torch.no_grad()
    def slerp(self, z_a, z_b, lambdas, node_mask):
        """[L,B,N,D]: spherical interpolation of two latents [B,N,D] per molecule at the weights `lambdas` (L floats; 0 returns z_a
        and 1 returns z_b bit for bit), in one library call (hd_slerp: angle and weights in double over the valid entries, the linear
        form where the latents are parallel; masked entries exactly 0, nothing re-centred)."""
        try:
            lam = [float(v) for v in (lambdas.reshape(-1).tolist() if isinstance(lambdas, (torch.Tensor, np.ndarray)) else lambdas)]
        except (TypeError, ValueError):
            raise ValueError(f"lambdas must be a sequence of numbers, got {lambdas!r}") from None
        if not lam or not all(math.isfinite(v) for v in lam):
            raise ValueError("lambdas must hold at least one finite weight")
        D = self.n_dims + self.in_node_nf
        if self.pocket:
            raise ValueError("slerp: pocket models are not supported (whole molecules only)")
        if not isinstance(node_mask, torch.Tensor) or node_mask.dim() != 3 or node_mask.shape[2] != 1:
            raise ValueError(f"node_mask must be [B, N, 1], got {tuple(getattr(node_mask, 'shape', ()))}")
        B, N = int(node_mask.shape[0]), int(node_mask.shape[1])
        for name, t in (("z_a", z_a), ("z_b", z_b)):
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != (B, N, D):
                raise ValueError(f"{name} must be [{B}, {N}, {D}], got {tuple(getattr(t, 'shape', ()))}")
        dev = node_mask.device
        if dev.type != "cuda":
            raise _lib.HierDiffHipError("editing runs only on an MI355X (no CPU fallback)")
        handle = self._lib_handle()
        topo = self.dynamics.topology(node_mask, None, B, N)
        za, zb = (t.detach().to(dev, torch.float32).contiguous() for t in (z_a, z_b))
        out = torch.empty((len(lam), B, N, D), device=dev, dtype=torch.float32)
        lam_c = (C.c_float * len(lam))(*lam)
        _lib.check(_lib.load().hd_slerp(handle, topo.ptr, za.data_ptr(), zb.data_ptr(), lam_c, len(lam), out.data_ptr(), _stream(dev)),
                   "hd_slerp")
        return out

    @torch.no_grad()
    def vary(self, samples: Sequence[Dict[str, torch.Tensor]], device, t_start, n_variants: int = 1, batch_size: int = 256,
             sample_id_base: int = 0, **few):
        """Variations of given molecules (the SDEdit idea): every molecule of `samples` (the sampler's result format, as `score`
        takes it) is noised to the grid index `t_start` (`diffuse`) and the reverse chain runs from there (`sample_from_latent`;
        keywords steps / eta / spacing / timesteps / solver / lower_order_final).  Returns `n_variants` results per input in the same format, input-major; variant
        v of input i runs under the sample id sample_id_base + i * n_variants + v, so it does not depend on the batch it ran in.
        guidance_scale (a float, or one scale per result, input-major) / guidance_rescale: classifier-free guidance of the reverse
        chain as in `sample_from_masks`, under the model's `null_context`.
        keep_frames / record: every result also holds 'chain_x' / 'chain_h' / 'chain_t' of its partial chain, as in `sample`.
        Mechanism only: how far which t_start drifts, and whether the analogues are chemically useful, is for the user to validate."""
        from . import scoring
        device = torch.device(device)
        extra = set(few) - set(KEYWORDS)
        if extra:
            raise ValueError(f"vary: unsupported keyword(s) {sorted(extra)} ({', '.join(KEYWORDS)})")
        if few.get("guidance_context") is not None:
            raise ValueError("vary: guidance_context is not supported (the list form pads its own batches): set the model's null_context")
        pl = self._plan("vary", "latent", t_start=t_start, **few)                       # argument errors first
        rr_all, gd_all, chain_t = pl.restraints, pl.guidance, pl.chain_t
        for k in ("restraints", "restraint_scale", "guidance_scale", "guidance_context"):  # per batch below: a slice of the resolved ones
            few.pop(k, None)
        for name, v in (("n_variants", n_variants), ("batch_size", batch_size)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or int(v) < 1:
                raise ValueError(f"{name} must be an integer >= 1, got {v!r}")
        if isinstance(sample_id_base, bool) or int(sample_id_base) != sample_id_base or int(sample_id_base) < 0:
            raise ValueError(f"sample_id_base must be an integer >= 0, got {sample_id_base!r}")
        samples = list(samples)
        if not samples:
            raise ValueError("vary: no samples")
        with_ctx = self.dynamics.context_node_nf > 0
        jobs = [mol for mol in samples for _ in range(int(n_variants))]
        if pl.steer is not None and (int(n_variants) % pl.steer.P or int(batch_size) % pl.steer.P):
            raise ValueError(f"vary: n_variants ({n_variants}) and batch_size ({batch_size}) must be multiples of particles "
                             f"({pl.steer.P}): the variants of one input form its groups")
        dv_all = pl.diversity
        if dv_all is not None:
            if int(n_variants) % dv_all.P or int(batch_size) % dv_all.P:
                raise ValueError(f"vary: n_variants ({n_variants}) and batch_size ({batch_size}) must be multiples of the diversity's "
                                 f"particles ({dv_all.P}): the variants of one input form its groups")
            if dv_all.scale.numel() not in (1, len(jobs) // dv_all.P):
                raise ValueError(f"vary: the diversity scale must hold one value per group ([{len(jobs) // dv_all.P}], input-major), got "
                                 f"{dv_all.scale.numel()}")
            few.pop("diversity", None)                                                  # per batch below: a slice of its scales
        if gd_all is not None and gd_all.rows != 1 and gd_all.rows != len(jobs):
            raise ValueError(f"vary: guidance_scale must hold one scale per result ([{len(jobs)}], input-major), got {gd_all.rows}")
        if rr_all is not None:
            rr_all.rs.check_batch(len(jobs), "vary (one set of rows per result, input-major)")
            if rr_all.scale.numel() not in (1, len(jobs)):
                raise ValueError(f"vary: restraint_scale must hold one scale per result ([{len(jobs)}], input-major), got "
                                 f"{rr_all.scale.numel()}")
        batches = [(lo, scoring.pad_samples(jobs[lo:lo + int(batch_size)], self.n_dims, self.in_node_nf, with_ctx))
                   for lo in range(0, len(jobs), int(batch_size))]
        self._edit_check("vary", batches[0][1][2], (), batches[0][1][3], needs_noise=True)
        out = []
        for lo, (x, h, nm, ctx) in batches:
            nmd, ctxd = nm.to(device), None if ctx is None else ctx.to(device)
            base = int(sample_id_base) + lo
            z = self.diffuse(x.to(device), h.to(device), nmd, t_start, sample_id_base=base)
            gs = None if gd_all is None else (float(gd_all.w[0]) if gd_all.rows == 1 else gd_all.w[lo:lo + nm.shape[0]])
            rk = {}
            if rr_all is not None:
                rk = dict(restraints=rr_all.rs.slice(lo, lo + nm.shape[0]),
                          restraint_scale=rr_all.scale if rr_all.scale.numel() == 1 else rr_all.scale[lo:lo + nm.shape[0]])
            if dv_all is not None:
                rk["diversity"] = dv_all.slice(lo // dv_all.P, (lo + nm.shape[0]) // dv_all.P)
            got = self.sample_from_latent(z, nmd, None, ctxd, t_start=t_start, sample_id_base=base, guidance_scale=gs, **few, **rk)
            ent = {} if rr_all is None else self._restraint_entries(rk["restraints"], rk["restraint_scale"], got[0], nmd, h=got[1])
            xv, hv = got[0].cpu(), got[1].cpu()
            part = []
            for i in range(nm.shape[0]):
                n = int(nm[i].sum())
                res = {'x': xv[i, :n].clone(), 'h': hv[i, :n].clone()}
                if ctx is not None:
                    res['context'] = ctx[i, :n].clone()
                restraints_mod.entries_into(res, ent, i, n)
                part.append(res)
            if chain_t is not None:
                self._chain_into(part, got[2], [int(nm[i].sum()) for i in range(nm.shape[0])], chain_t)
            if pl.steer is not None:
                steering_mod.into(part, self.steer_last, group0=lo // pl.steer.P)
            if dv_all is not None:
                diversity_mod.into(part, self.diversity_last, group0=lo // dv_all.P)
            out.extend(part)
        return out

    @torch.no_grad()
    def interpolate(self, sample_a: Dict[str, torch.Tensor], sample_b: Dict[str, torch.Tensor], frames: int, device, *,
                    t_end: Optional[int] = None, steps: Optional[int] = None, spacing: Optional[str] = None, restraints=None):
        """`frames` molecules between two of equal node count (the sampler's result format; ValueError otherwise): both are encoded
        to z_{t_end} (`encode`), the latents interpolated on the sphere at lambda = i / (frames - 1) (`slerp`), and every frame decoded
        with eta = 0 on the reversed path (`sample_from_latent`), all frames as one batch that shares the decode's noise row - so
        frames 0 and frames - 1 are the eta = 0 reconstructions of the two inputs, bit for bit.  A context is interpolated linearly.
        Returns a list of `frames` results.  Mechanism only: what lies between two molecules is a property of the weights."""
        from . import scoring, restraints as _rs
        _rs.refuse(self, "interpolate", restraints, ": its frames are reconstructions of the interpolated latents")
        steering_mod.refuse(self, "interpolate")
        diversity_mod.refuse(self, "interpolate", None, ": its frames are reconstructions of the interpolated latents")
        corrector_mod.refuse(self, "interpolate", None, ": its frames are reconstructions of the interpolated latents")
        device = torch.device(device)
        if isinstance(frames, bool) or not isinstance(frames, (int, np.integer)) or int(frames) < 2:
            raise ValueError(f"frames must be an integer >= 2, got {frames!r}")
        L = int(frames)
        from . import paths
        t_end_i = self._grid_index(self.T if t_end is None else t_end, 1, "t_end")
        paths.partial_path(self.T, t_end_i, steps, self.sample_spacing if spacing is None else spacing)        # argument errors first
        with_ctx = self.dynamics.context_node_nf > 0
        x, h, nm, ctx = scoring.pad_samples([sample_a, sample_b], self.n_dims, self.in_node_nf, with_ctx)
        if int(nm[0].sum()) != int(nm[1].sum()):
            raise ValueError(f"interpolate: the molecules must have equal node counts, got {int(nm[0].sum())} and {int(nm[1].sum())}")
        self._edit_check("interpolate", nm, (), ctx, needs_noise=True)
        nmd = nm.to(device)
        z = self.encode(x.to(device), h.to(device), nmd, None, None if ctx is None else ctx.to(device), t_end=t_end_i, steps=steps,
                        spacing=spacing)
        lam = [i / (L - 1) for i in range(L)]
        zf = self.slerp(z[0:1], z[1:2], lam, nmd[0:1]).reshape(L, z.shape[1], z.shape[2])
        nm_f = nmd[0:1].expand(L, -1, -1).contiguous()
        ctx_f = None
        if ctx is not None:
            w = torch.tensor(lam, dtype=torch.float32).view(L, 1, 1)
            ctx_f = ((1.0 - w) * ctx[0:1] + w * ctx[1:2]).contiguous()
        xf, hf = self.sample_from_latent(zf, nm_f, None, None if ctx_f is None else ctx_f.to(device), t_start=t_end_i, steps=steps,
                                         eta=0.0, spacing=spacing, fix_noise=True, solver="ddim")
        xf, hf = xf.cpu(), hf.cpu()
        n = int(nm[0].sum())
        out = []
        for i in range(L):
            res = {'x': xf[i, :n].clone(), 'h': hf[i, :n].clone()}
            if ctx_f is not None:
                res['context'] = ctx_f[i, :n].clone()
            out.append(res)
        return out

    # ------------------------------------------------------------------ fragment-constrained sampling (no reference counterpart)
    def _inpaint_schedule(self, handle, tabs):
        """{alpha_s, sigma_s, alpha_t|s, sigma_t|s} per step from the gamma grid of `_schedule`, uploaded once per table."""
        if self.__dict__.get("_inpaint_tabs") is not tabs:
            g = tabs["gamma"].to(torch.float32).reshape(-1)[:-1]
            coef = tabs["coef"]
            rows = torch.stack([torch.sqrt(torch.sigmoid(-g)), torch.sqrt(torch.sigmoid(g)), coef[:, 0], torch.sqrt(coef[:, 1])], dim=1)
            rows = np.ascontiguousarray(rows.numpy(), dtype=np.float32)
            _lib.check(_lib.load().hd_set_inpaint_schedule(handle, self.T, rows.ctypes.data_as(C.POINTER(C.c_float))),
                       "hd_set_inpaint_schedule")
            self._inpaint_tabs = tabs
        return tabs

    def _inpaint_setup(self, node_mask, fixed_mask, x_known, h_known, context, resamplings, edge_mask, pl=None, fixed_x_mask=None,
                       fixed_h_mask=None):
        """Argument checks of the inpainting entry points (ValueError / NotImplementedError before anything is queued), then the
        device state with the inpainting extras on top: the fixed rows' mask bytes, their known values (normalised) and R.  `pl`: the
        call's plan (None: the model's path defaults, unguided - `inpaint_steps`).  fixed_x_mask / fixed_h_mask: partial masks
        (each defaults to `fixed_mask`); then `fm_u8` is the position mask and `fh_u8` [B*N*F] the channel mask (else None)."""
        if node_mask.dim() != 3 or node_mask.shape[2] != 1:
            raise ValueError(f"node_mask must be [B, N, 1], got {tuple(node_mask.shape)}")
        B, N = int(node_mask.shape[0]), int(node_mask.shape[1])
        F_ = self.in_node_nf
        parts = fixed_x_mask is not None or fixed_h_mask is not None
        if fixed_mask is None:
            if fixed_x_mask is None or fixed_h_mask is None:
                raise ValueError("fixed_mask may be None only when fixed_x_mask and fixed_h_mask are both given")
        elif tuple(fixed_mask.shape) != (B, N, 1):
            raise ValueError(f"fixed_mask must be [{B}, {N}, 1], got {tuple(fixed_mask.shape)}")
        if parts:
            fixed_x_mask = fixed_mask if fixed_x_mask is None else fixed_x_mask
            fixed_h_mask = fixed_mask if fixed_h_mask is None else fixed_h_mask
            if tuple(fixed_x_mask.shape) != (B, N, 1):
                raise ValueError(f"fixed_x_mask must be [{B}, {N}, 1], got {tuple(fixed_x_mask.shape)}")
            if tuple(fixed_h_mask.shape) not in ((B, N, 1), (B, N, F_)):
                raise ValueError(f"fixed_h_mask must be [{B}, {N}, 1] or [{B}, {N}, {F_}], got {tuple(fixed_h_mask.shape)}")
        if tuple(x_known.shape) != (B, N, self.n_dims):
            raise ValueError(f"x_known must be [{B}, {N}, {self.n_dims}], got {tuple(x_known.shape)}")
        if tuple(h_known.shape) != (B, N, F_):
            raise ValueError(f"h_known must be [{B}, {N}, {F_}], got {tuple(h_known.shape)}")
        if isinstance(resamplings, bool) or int(resamplings) != resamplings or int(resamplings) < 1:
            raise ValueError(f"resamplings must be an integer >= 1, got {resamplings!r}")
        if (self.T + 2) * 3 * int(resamplings) >= 2 ** 32:
            raise ValueError("(timesteps + 2) * 3 * resamplings exceeds the generator's 32-bit draw index")
        dev = node_mask.device
        nmb = node_mask.to(torch.bool)
        if parts:
            fmb = fixed_x_mask.to(dev).to(torch.bool)
            fhb = fixed_h_mask.to(dev).to(torch.bool).expand(B, N, F_)
            if bool((fmb & ~nmb).any()):
                raise ValueError("fixed_x_mask must be a subset of node_mask")
            if bool((fhb & ~nmb).any()):
                raise ValueError("fixed_h_mask must be a subset of node_mask")
        else:
            fmb = fixed_mask.to(dev).to(torch.bool)
            if bool((fmb & ~nmb).any()):
                raise ValueError("fixed_mask must be a subset of node_mask")
        if edge_mask is not None and edge_mask.numel() != B * N * N:
            raise ValueError(f"edge_mask must hold {B} x {N} x {N} entries")
        if self.dynamics.context_node_nf > 0 and context is None:
            raise ValueError("context required")
        unsupported(self, "inpainting", None, True)
        if pl is None:
            pl = self._plan("inpainting", "inpaint", guided=False)
        st = self._device_state(node_mask, edge_mask, context, B, N, pl, inpaint=True)
        xk = x_known.to(dev, torch.float32).contiguous()
        hk = h_known.to(dev, torch.float32).contiguous()
        # the model's own `normalize`, masked by the fixed rows (the library ignores the others)
        xh_known = torch.cat([xk / float(self.norm_values[0]),
                              (hk - float(self.norm_biases[1] or 0.0)) / float(self.norm_values[1])], dim=2)
        keep = torch.cat([fmb.expand(B, N, self.n_dims), fhb], dim=2) if parts else fmb
        xh_known = torch.where(keep, xh_known, torch.zeros_like(xh_known)).contiguous()
        fm_u8 = fmb.reshape(B * N).to(torch.uint8).contiguous()
        fh_u8 = fhb.reshape(B * N * F_).to(torch.uint8).contiguous() if parts else None
        st.update(pl=pl, xk=xk, hk=hk, xh_known=xh_known, fm_u8=fm_u8, fh_u8=fh_u8, R=int(resamplings),
                  K=None if pl.path is None else pl.K)
        return st

    @torch.no_grad()
    def inpaint_steps(self, z, s_hi: int, s_lo: int, node_mask, fixed_mask, x_known, h_known, context=None, resamplings: int = 1,
                      sample_id_base: int = 0, edge_mask=None, *, restraints=None, restraint_scale=None, restraint_schedule=None,
                      restraint_clip=None, restraint_frame: Optional[str] = None, fixed_x_mask=None, fixed_h_mask=None):
        """The steps s = s_hi-1 ... s_lo of `sample_inpaint`'s loop on a given z_{s_hi} [B,N,D] (normalised units); returns z_{s_lo}.
        fixed_x_mask / fixed_h_mask: partial masks, as in `sample_inpaint`.
        Draws are keyed by the step, so a chain cut into pieces gives the bits of the whole.  restraint_frame="known" (or the
        model's `restraint_frame`): the restraints of `sample_inpaint`, on the path loop; without it the restraint keywords and the
        model's restraint attributes are ignored, as they always were."""
        from . import restraints as _rs
        pl = None
        if _rs.check_frame(self, restraint_frame):
            B, N = self._batch_of(node_mask)
            pl = self._plan("inpaint_steps", "inpaint", B=B, N=N, guided=False, **given(locals()))
        st = self._inpaint_setup(node_mask, fixed_mask, x_known, h_known, context, resamplings, edge_mask, pl, fixed_x_mask, fixed_h_mask)
        if tuple(z.shape) != (st.B, st.N, self.n_dims + self.in_node_nf) or not (0 <= s_lo <= s_hi <= self.T):
            raise ValueError("z must be [B, N, 3 + F] and 0 <= s_lo <= s_hi <= timesteps")
        z = z.detach().to(st.dev, torch.float32).clone().contiguous()
        n_loop = st.pl.K                                 # s counts path positions from the t = 0 end (the grid itself by default)
        return self._run(st, st.pl, z, n_loop - int(s_hi), n_loop - int(s_lo), (None, None, st.B, self.seed, sample_id_base),
                         (st.fm_u8, st.xh_known, st.R, st.fh_u8))[0]

    @torch.no_grad()
    def sample_inpaint(self, node_mask: torch.Tensor, fixed_mask: torch.Tensor, x_known: torch.Tensor, h_known: torch.Tensor,
                       context=None, resamplings: int = 1, sample_id_base: int = 0, edge_mask: Optional[torch.Tensor] = None, *,
                       steps: Optional[int] = None, eta: Optional[float] = None, spacing: Optional[str] = None,
                       timesteps: Optional[Sequence[int]] = None, guidance_scale=None, guidance_context=None, guidance_rescale: Optional[float] = None,
                       solver: Optional[str] = None, keep_frames: Optional[int] = None, record: Optional[str] = None,
                       restraints=None, restraint_scale=None, restraint_schedule=None, restraint_clip=None,
                       restraint_frame: Optional[str] = None, fixed_x_mask=None, fixed_h_mask=None):
        """(x, h) on the device for molecules whose `fixed_mask` [B,N,1] nodes are known: `x_known` [B,N,3] / `h_known` [B,N,F] in
        data units (what `sample` returns; rows outside `fixed_mask` are ignored, the frame of the positions is free).  The free
        nodes are sampled around them by the replacement method, `resamplings` network calls per step (RePaint for > 1), inside
        the library's loop (hd_sample_loop_inpaint; algorithm and draw layout in include/hierdiff_hip.h).  Returned fixed rows:
        h = h_known exactly, x = x_known translated as one block.  Training-free conditioning: how well the free part fits the
        known one depends on the model and on `resamplings`.  A sample depends on its global id (sample_id_base + row), its
        masks, the weights and its known values only.  steps / spacing / timesteps: few-step sampling as in `sample_from_masks`
        (hd_sample_path_inpaint), ancestral steps only - eta < 1 raises ValueError.  guidance_scale / guidance_context /
        guidance_rescale: classifier-free guidance as in `sample_from_masks` (every round's network call is guided).
        solver="dpm2m" or "sde2m" (or the model's `sample_solver`) raises ValueError like eta < 1.  keep_frames / record: as in
        `sample_from_masks` - a third tensor chain [keep_frames, B, N, D]; a frame is the state behind its transition's last round
        (known rows replaced), or that round's data prediction, and frame 0 the returned (x, h).
        restraint_frame="known" (or the model's `restraint_frame`): restraints / restraint_scale / restraint_schedule / restraint_clip
        as in `sample_from_masks`, with the tables read in the frame of `x_known` as given (hierdiff_amd/restraints.py, THE FRAME):
        "grow this fragment without clashing with these protein atoms" in the pocket's own coordinates.  Free nodes only are pushed;
        the update runs in every resampling round, behind guidance, on the path loop (the identity path where the keywords ask
        for the plain loop).  The call then returns one more element, a dict with 'restraint_energy' [B,3] float64 (evaluated in
        the known frame), 'frame_shift' [B,3] float64 (the translation tau of the returned x) and 'x_known_frame' [B,N,3] = x - tau,
        the molecule in the coordinates of the input (known rows equal `x_known` up to fp32 rounding).  Without it restraints are
        refused, as before: the model's frame moves with the known fragments.
        PARTIAL MASKS: fixed_x_mask [B,N,1] ("the position of this node is known") and fixed_h_mask [B,N,1] or [B,N,F] ("this
        feature channel of this node is known") replace `fixed_mask` part by part; each defaults to `fixed_mask`, which may be None
        when both are given.  Features known and positions free lays a given bag of fragments out in 3-D; positions known and features
        (or some channels) free fills a given shape.  Rows / channels of x_known / h_known outside their mask are ignored.  Returned:
        h = h_known exactly on the known channels, x = x_known translated as one block on the position-known nodes; everything else is
        sampled.  Position components of a node are known together.  With restraint_frame="known" the frame, 'frame_shift' and
        'x_known_frame' belong to the position-known nodes; a node with known features and a free position is free and is pushed, and
        a molecule without position-known nodes reads the tables in the model's frame (tau = 0).  A mechanism only: how well free
        positions fit known features, and which `resamplings` helps, depends on the checkpoint."""
        from . import restraints as _rs
        if not _rs.check_frame(self, restraint_frame):
            _rs.refuse(self, "sample_inpaint", restraints, ": inpainting re-centres on the known fragments, so its frame moves")
        steering_mod.refuse(self, "sample_inpaint")
        B, N = self._batch_of(node_mask)
        pl = self._plan("sample_inpaint", "inpaint", B=B, N=N, **given(locals()))            # every keyword error before any shape check
        st = self._inpaint_setup(node_mask, fixed_mask, x_known, h_known, context, resamplings, edge_mask, pl, fixed_x_mask, fixed_h_mask)
        z = torch.empty((st.B, st.N, self.n_dims + self.in_node_nf), device=st.dev, dtype=torch.float32)
        _lib.check(_lib.load().hd_noise(st.h, st.topo.ptr, None, None, st.B, self.seed, sample_id_base, 0, 0, z.data_ptr(), st.stream),
                   "hd_noise")
        noise, inp = (None, None, st.B, self.seed, sample_id_base), (st.fm_u8, st.xh_known, st.R, st.fh_u8)
        if self.debug_checks:              # the loop's invariant after every step (host-synchronising, like the reference's asserts)
            for k in range(pl.K):
                z, chain = self._run(st, pl, z, k, k + 1, noise, inp)
                self._check_mean_zero(z[:, :, :self.n_dims], node_mask)
        else:
            z, chain = self._run(st, pl, z, 0, pl.K, noise, inp)
        got = self._decode(st, z, node_mask, edge_mask, False, int(sample_id_base), chain, (st.fm_u8, st.xk, st.hk, st.fh_u8))
        rr = pl.restraints
        if rr is None or not rr.frame:
            return got
        info = self._restraint_entries(rr.rs, rr.scale, got[0], node_mask, st.fm_u8, st.xk, cpu=False, h=got[1])
        tau = info['frame_shift']
        info['x_known_frame'] = ((got[0].double() - tau[:, None, :]) * node_mask.to(st.dev, torch.float64)).to(torch.float32)
        return tuple(got) + (info,)

    @torch.no_grad()
    def sample_grow(self, known: Sequence[Dict[str, torch.Tensor]], sizes, device, context=None, resamplings: int = 1,
                    sample_id_base: int = 0, *, steps: Optional[int] = None, eta: Optional[float] = None,
                    spacing: Optional[str] = None, timesteps: Optional[Sequence[int]] = None, guidance_scale=None, guidance_context=None, guidance_rescale: Optional[float] = None,
                    solver: Optional[str] = None, keep_frames: Optional[int] = None, record: Optional[str] = None,
                    restraints=None, restraint_scale=None, restraint_schedule=None, restraint_clip=None,
                    restraint_frame: Optional[str] = None):
        """List-level form of `sample_inpaint` in `sample`'s result format: `known[i]` = {'x': [k_i,3], 'h': [k_i,F]} are the fragments
        molecule i keeps (its first k_i rows in the result; k_i = 0 allowed), `sizes[i]` >= k_i its total number of fragments (one
        integer: that many for every molecule).  `context`: as in `sample`.  Returns [{'x': [n_i,3], 'h': [n_i,F] (, 'context')}] on
        the CPU.  steps / eta / spacing / timesteps: as in `sample_inpaint`.  keep_frames / record: every dict also holds 'chain_x'
        [keep, n_i, 3], 'chain_h' [keep, n_i, F] and 'chain_t' [keep], as in `sample`.  restraint_frame="known" with restraints /
        restraint_scale (a float or a [len(known)] tensor) / restraint_schedule / restraint_clip: as in `sample_inpaint`, the tables
        in the coordinates of the given fragments; every dict then also holds 'restraint_energy' [3] float64, 'frame_shift' [3]
        float64 and 'x_known_frame' [n_i, 3].
        PARTIAL KNOWLEDGE: known[i] may hold 'x' only (positions known, features sampled), 'h' only (features known, positions
        sampled) or both, and optional boolean 'x_mask' [k_i] / 'h_mask' [k_i] or [k_i, F] that narrow them to some rows / channels;
        k_i is the row count of whichever of 'x' / 'h' is there.  Entries with both and no masks make the whole-node call, as before."""
        device = torch.device(device)
        from . import restraints as _rs
        if not _rs.check_frame(self, restraint_frame):
            _rs.refuse(self, "sample_grow", restraints, ": inpainting re-centres on the known fragments, so its frame moves")
        steering_mod.refuse(self, "sample_grow")
        few = given(locals())
        framed = _rs.check_frame(self, restraint_frame)
        pl0 = self._plan("sample_grow", "inpaint", **(dict(B=len(known) or None) if framed else {}), **few)     # argument errors first
        chain_t = pl0.chain_t
        num = len(known)
        if isinstance(sizes, (int, np.integer)):
            sizes = [int(sizes)] * num
        sizes = [int(n) for n in sizes]
        if len(sizes) != num or num == 0:
            raise ValueError("sizes must hold one total size per known molecule (and there must be at least one)")
        ks, F_ = [], self.in_node_nf
        parts = any(mol.get("x") is None or mol.get("h") is None or mol.get("x_mask") is not None or mol.get("h_mask") is not None
                    for mol in known)
        for i, mol in enumerate(known):
            kx = None if mol.get("x") is None else torch.as_tensor(mol["x"])
            kh = None if mol.get("h") is None else torch.as_tensor(mol["h"])
            if kx is None and kh is None:
                raise ValueError(f"known[{i}]: need 'x' [k, {self.n_dims}] or 'h' [k, {F_}] (or both)")
            k = int((kx if kx is not None else kh).shape[0])
            if (kx is not None and (kx.dim() != 2 or kx.shape[1] != self.n_dims)) or \
                    (kh is not None and (kh.dim() != 2 or tuple(kh.shape) != (k, F_))):
                raise ValueError(f"known[{i}]: need 'x' [k, {self.n_dims}] and 'h' [k, {F_}]")
            if mol.get("x_mask") is not None and (kx is None or tuple(torch.as_tensor(mol["x_mask"]).shape) != (k,)):
                raise ValueError(f"known[{i}]: 'x_mask' must be [{k}] and go with 'x'")
            if mol.get("h_mask") is not None and (kh is None or tuple(torch.as_tensor(mol["h_mask"]).shape) not in ((k,), (k, F_))):
                raise ValueError(f"known[{i}]: 'h_mask' must be [{k}] or [{k}, {F_}] and go with 'h'")
            if sizes[i] < max(1, k):
                raise ValueError(f"known[{i}]: total size {sizes[i]} is smaller than its {k} known fragments (or zero)")
            ks.append(k)
        n_max = max(sizes)
        ar = torch.arange(n_max)
        node_mask = (ar[None, :] < torch.tensor(sizes)[:, None]).unsqueeze(-1)
        fixed_mask = (ar[None, :] < torch.tensor(ks)[:, None]).unsqueeze(-1)
        x_known = torch.zeros(num, n_max, self.n_dims)
        h_known = torch.zeros(num, n_max, F_)
        fx_mask = torch.zeros(num, n_max, 1, dtype=torch.bool)
        fh_mask = torch.zeros(num, n_max, F_, dtype=torch.bool)
        for i, mol in enumerate(known):
            if mol.get("x") is not None:
                x_known[i, :ks[i]] = torch.as_tensor(mol["x"], dtype=torch.float32)
                xm = mol.get("x_mask")
                fx_mask[i, :ks[i], 0] = True if xm is None else torch.as_tensor(xm).to(torch.bool)
            if mol.get("h") is not None:
                h_known[i, :ks[i]] = torch.as_tensor(mol["h"], dtype=torch.float32)
                hm = mol.get("h_mask")
                fh_mask[i, :ks[i]] = True if hm is None else torch.as_tensor(hm).to(torch.bool).reshape(ks[i], -1)
        part_kw = dict(fixed_x_mask=fx_mask.to(device), fixed_h_mask=fh_mask.to(device)) if parts else {}
        ctx = None
        if context is not None:
            ctx = torch.zeros([num, n_max, 1]) + torch.as_tensor(context, dtype=torch.float32).cpu()
            if ctx.shape != (num, n_max, 1):
                raise ValueError(f"context of shape {tuple(torch.as_tensor(context).shape)} does not broadcast to [{num}, {n_max}, 1]")
        got = self.sample_inpaint(node_mask.to(device), fixed_mask.to(device), x_known.to(device), h_known.to(device),
                                  context=None if ctx is None else ctx.to(device), resamplings=resamplings,
                                  sample_id_base=sample_id_base, **few, **part_kw)
        x, h = got[0].cpu(), got[1].cpu()
        out = [{'x': x[i, :sizes[i]].clone(), 'h': h[i, :sizes[i]].clone()} for i in range(num)]
        if ctx is not None:
            for i in range(num):
                out[i]['context'] = ctx[i, :sizes[i]].clone()
        if chain_t is not None:
            self._chain_into(out, got[2], sizes, chain_t)
        if pl0.restraints is not None:
            info = {k: v.cpu() for k, v in got[-1].items()}
            for i in range(num):
                restraints_mod.entries_into(out[i], info, i, sizes[i])
        return out

    @torch.no_grad()
    def sample(self, num_samples, device, context=None, pocket_cond=None, sample_id_base: int = 0, *,
               steps: Optional[int] = None, eta: Optional[float] = None, spacing: Optional[str] = None,
               timesteps: Optional[Sequence[int]] = None, guidance_scale=None, guidance_context=None, guidance_rescale: Optional[float] = None,
               solver: Optional[str] = None, lower_order_final: Optional[bool] = None,
               keep_frames: Optional[int] = None, record: Optional[str] = None,
               restraints=None, restraint_scale=None, restraint_schedule=None, restraint_clip=None,
               particles=None, steer_scale=None, steer_ess=None, steer_schedule=None, restraint_frame=None, diversity=None, corrector=None):
        """diffusion_qm9.py:347-395: list of {'x': [n_i,3], 'h': [n_i,8], ('context': [n_i,1])} on the CPU.
        steps / eta / spacing / timesteps: few-step sampling, see `sample_from_masks`; guidance_scale (a float or a
        [num_samples] tensor) / guidance_context ([num_samples, n_max, C]) / guidance_rescale: classifier-free guidance, ibid.;
        solver / lower_order_final: "dpm2m" / "sde2m" = second-order multistep sampling, ibid.
        keep_frames / record ("z", the default, or "x0"): the trajectory, ibid. - every dict also holds 'chain_x' [keep, n_i, 3],
        'chain_h' [keep, n_i, F] (CPU, data units, the reference's frame order: frame 0 is the result itself) and 'chain_t' [keep],
        the grid index every frame's state had arrived at.
        restraints / restraint_scale (a float or a [num_samples] tensor) / restraint_schedule / restraint_clip: restraint-guided
        sampling, ibid. (tables with a batch axis hold num_samples sets of rows; coordinates in the model's frame, the molecule's
        centre of mass at the origin) - every dict also holds 'restraint_energy', float64 [3] = (U_obs, U_pair, U_anc) of the
        returned 'x'.  The sizes are drawn: a row that names a node the molecule does not have is inactive."""
        device = torch.device(device)
        few = given(locals())
        pl = self._plan("sample", pocket=pocket_cond, B=int(num_samples), **few)         # argument errors before anything is drawn
        if pl.guidance is not None and context is None:
            raise ValueError("context required")
        if pl.steer is not None:                         # one size per group, P times: the particles of a group share their mask
            sample_n = [n for n in self.nodes_dist.sample(int(num_samples) // pl.steer.P) for _ in range(pl.steer.P)]
        elif pl.diversity is not None:                   # ... and so do the rows of a diverse group
            sample_n = [n for n in self.nodes_dist.sample(int(num_samples) // pl.diversity.P) for _ in range(pl.diversity.P)]
        else:
            sample_n = self.nodes_dist.sample(num_samples)
        pocket = None
        if pocket_cond is not None:
            if not self.pocket:
                raise ValueError("pocket_cond given but the model was built with cfg.pocket = False")
            pocket = (pocket_cond[1].to(device, torch.float32),
                      self.pocket_embed(pocket_cond[0].to(device).long()).to(torch.float32),
                      pocket_cond[2].to(device).bool(), pocket_cond[3].to(device).bool())
        ctx = None
        if context is not None:
            # `zeros([num_samples, n_max, 1]) + context` (:352): a scalar, or any tensor that broadcasts against that shape
            # (e.g. one value per sample as [num_samples, 1, 1]); anything else raises here as it does there
            ctx = torch.zeros([num_samples, max(sample_n), 1]) + torch.as_tensor(context, dtype=torch.float32).cpu()
            if ctx.shape != (num_samples, max(sample_n), 1):
                raise ValueError(f"context of shape {tuple(torch.as_tensor(context).shape)} does not broadcast to "
                                 f"[{num_samples}, {max(sample_n)}, 1]")
        return self._sample_sizes(sample_n, device, None, sample_id_base, pocket, context_full=ctx, few=few, pl=pl)

    def _sample_sizes(self, sample_n, device, contexts, sample_id_base, pocket=None, context_full=None, few=None, pl=None):
        """One device batch for the molecule sizes `sample_n` (global sample ids sample_id_base + i); `contexts`: one scalar
        per molecule (merged batches: the value of the batch a molecule belongs to) or None; `context_full`: the
        [num_samples, n_max, 1] tensor of `sample()` instead.  Masks as diffusion_qm9.py:349-353, result slicing as :388-395."""
        num_samples = len(sample_n)
        n_max = max(sample_n)
        sizes = torch.tensor(sample_n)
        ar = torch.arange(n_max)
        node_mask = (ar[None, :] < sizes[:, None]).unsqueeze(-1)
        context = None
        if context_full is not None:
            context = context_full.to(device)
        elif contexts is not None:
            cols = [torch.as_tensor(c, dtype=torch.float32).reshape(-1).cpu() for c in contexts]
            if any(c.numel() != 1 for c in cols):
                raise ValueError("merged batches take one global context value per batch (context_range entries)")
            context = (torch.zeros([num_samples, n_max, 1]) + torch.stack(cols).reshape(num_samples, 1, 1)).to(device)
        node_mask = node_mask.to(device)
        few = few or {}
        if pl is None:                               # (`sample` passes its plan; merged `sample_batches` batches come without one)
            pl = self._plan("sample", pocket=pocket, B=num_samples, **few)
        got = self.sample_from_masks(node_mask, None, context, sample_id_base=sample_id_base, pocket=pocket, **few)
        x, h = got[0].cpu(), got[1].cpu()
        xs = [x[i, :sample_n[i]].clone() for i in range(num_samples)]
        hs = [h[i, :sample_n[i]].clone() for i in range(num_samples)]
        if context is not None:
            ctx = context.cpu()
            out = [{'x': xs[i], 'h': hs[i], 'context': ctx[i, :sample_n[i]].clone()} for i in range(num_samples)]
        else:
            out = [{'x': xs[i], 'h': hs[i]} for i in range(num_samples)]
        if len(got) == 3:                            # a recording call (`sample`: keep_frames)
            self._chain_into(out, got[2], sample_n, pl.chain_t)
        rr = pl.restraints
        if rr is not None:
            ent = self._restraint_entries(rr.rs, rr.scale, got[0], node_mask, h=got[1])
            for i in range(num_samples):
                restraints_mod.entries_into(out[i], ent, i, sample_n[i])
        if pl.steer is not None:
            steering_mod.into(out, self.steer_last)
        if pl.diversity is not None:
            diversity_mod.into(out, self.diversity_last)
        return out

    def sample_batches(self, batch_size, num_batches, device, context_range=None, protein_data_all=None,
                       sample_id_base: int = 0, *, steps: Optional[int] = None, eta: Optional[float] = None,
                       spacing: Optional[str] = None, timesteps: Optional[Sequence[int]] = None, guidance_scale=None, guidance_context=None, guidance_rescale: Optional[float] = None,
                       solver: Optional[str] = None, lower_order_final: Optional[bool] = None, restraints=None):
        """diffusion_qm9.py:397-436, incl. the protein branch (`protein_data_all`: list of dicts with
        'residue_type', 'coord', 'pocket_name', 'ligand_name').

        The reference runs the batches one after the other (its shipped job is 16 batches of 2 molecules,
        conf/sample/default.yaml:1-2).  Molecules are independent, and here a sample's bits depend only on its global id
        (counter RNG keyed by the id, per-molecule tiles, batch-size-independent kernels), so consecutive batches are run
        as one device batch of at most `self.merge_batches` molecules / `self.merge_edges` directed edges: same results, bit for bit, as the loop
        (tests/test_gpu_configs.py::test_merged_sample_batches_equal_the_loop), at the throughput of the larger batch.
        The molecule sizes are drawn batch by batch exactly as the loop draws them.  Not merged: the protein branch,
        `noise_mode == "torch"` (torch.randn draws depend on the batch shape), `merge_batches = 0`, and the two
        configurations whose results depend on a batch's padded width (below).  One difference that
        is not a sample's own: the NaN guard (en_dynamics.py:109-111) zeroes the velocity of the whole DEVICE batch."""
        device = torch.device(device)
        from . import restraints as _rs
        _rs.refuse(self, "sample_batches", restraints, ": the batches' padded widths and molecule counts differ (use sample)")
        steering_mod.refuse(self, "sample_batches")
        diversity_mod.refuse(self, "sample_batches", None, ": the batches' molecule counts differ (use sample)")
        corrector_mod.refuse(self, "sample_batches", None, " (use sample)")
        # classifier-free guidance (`sample_from_masks`): guidance_scale may also be a list / tuple of scales cycled per batch the way
        # context_range is; inside a merged device batch it becomes one scale per molecule
        from . import guidance
        gscale = self.guidance_scale if guidance_scale is None else guidance_scale
        if guidance_context is not None:
            raise ValueError("sample_batches: guidance_context is not supported (the batches' padded widths differ): set the "
                             "model's null_context")
        if isinstance(gscale, (torch.Tensor, np.ndarray)) and gscale.ndim > 0:
            raise ValueError("sample_batches: guidance_scale must be a float or a list / tuple of floats cycled per batch")
        g_seq = guidance.batch_scales(gscale, int(num_batches), int(batch_size)) if guidance.is_sequence_scale(gscale) else None
        few = given(dict(locals(), guidance_scale=gscale if g_seq is None else None))
        self._plan("sample_batches", pocket=protein_data_all,                            # few-step sampling, guidance: argument errors first
                   **dict(few, **({} if g_seq is None else {"guidance_scale": torch.tensor(g_seq)})))
        # Not merged either: mode 'gnn_dynamics' (torch.randn draws whatever noise_mode says, messages over padded nodes) and
        # aggregation_method 'mean' (the divisor is the padded N of the call) - both depend on the padded width of the batch a
        # molecule sits in - and context_range entries that are not one scalar per batch.
        width_dependent = (getattr(self.dynamics, "mode", "egnn_dynamics") == "gnn_dynamics"
                           or getattr(self.dynamics, "aggregation_method", "sum") == "mean")
        scalar_ctx = context_range is None or all(torch.as_tensor(c).numel() == 1 for c in context_range)
        if (protein_data_all is None and self.merge_batches and self.noise_mode == "philox" and num_batches > 1
                and not width_dependent and scalar_ctx):
            sizes, ctxs = [], []
            for i in range(num_batches):
                sizes.extend(self.nodes_dist.sample(batch_size))
                if context_range is not None:
                    ctxs.extend([context_range[i % len(context_range)]] * batch_size)
            bs = int(batch_size)
            results, lo = [], 0
            while lo < len(sizes):                              # whole batches, greedily, within both limits
                hi, edges = lo + bs, sum(n * (n - 1) for n in sizes[lo:lo + bs])
                while hi < len(sizes):
                    more = sum(n * (n - 1) for n in sizes[hi:hi + bs])
                    if hi + bs - lo > int(self.merge_batches) or (self.merge_edges and edges + more > int(self.merge_edges)):
                        break
                    hi, edges = hi + bs, edges + more
                few_m = dict(few)
                if g_seq is not None:                          # one scale per molecule: that of the batch it belongs to
                    few_m["guidance_scale"] = torch.tensor([g_seq[j // bs] for j in range(lo, hi)], dtype=torch.float32)
                results.extend(self._sample_sizes(sizes[lo:hi], device, ctxs[lo:hi] if ctxs else None, sample_id_base + lo,
                                                  **({"few": few_m} if few_m else {})))
                lo = hi
            return results, []
        protein_cond_all = None
        if protein_data_all is not None:
            protein_cond_all = pocket_tensors(protein_data_all)
        results, test_names = [], []
        for i in range(num_batches):
            lo, hi = i * batch_size, (i + 1) * batch_size
            base = sample_id_base + lo
            if g_seq is not None:                              # per molecule, as in the merged run (a scalar 1.0 would be unguided)
                few = dict(few, guidance_scale=torch.full((int(batch_size),), g_seq[i], dtype=torch.float32))
            if protein_cond_all is not None:
                n_prot = len(protein_cond_all[0])
                cond = [x[lo % n_prot: (hi - 1) % n_prot + 1] for x in protein_cond_all]
                # the reference indexes the names modulo len(protein_cond_all) == 4 (diffusion_qm9.py:428); kept as is
                names = [protein_data_all[k]['pocket_name'] + '/' + protein_data_all[k]['ligand_name']
                         for k in range(lo % len(protein_cond_all), hi % len(protein_cond_all))]
                results.extend(self.sample(batch_size, device, context=None, pocket_cond=cond, sample_id_base=base, **few))
                test_names.extend(names)
            elif context_range is not None:
                results.extend(self.sample(batch_size, device, context=context_range[i % len(context_range)],
                                           pocket_cond=None, sample_id_base=base, **few))
            else:
                results.extend(self.sample(batch_size, device, context=None, pocket_cond=None, sample_id_base=base, **few))
        return results, test_names


class EnVariationalDiffusion(DiffusionQM9):
    """EDM-style entry point (en_diffusion.py:634-667): masks supplied by the caller, fix_noise honoured."""

    @torch.no_grad()
    def sample(self, n_samples, n_nodes, node_mask, edge_mask, context, fix_noise=False, *,  # type: ignore[override]
               steps=None, eta=None, spacing=None, timesteps=None, guidance_scale=None, guidance_context=None, guidance_rescale=None,
               solver=None, lower_order_final=None, corrector=None):
        assert node_mask.shape[0] == n_samples and node_mask.shape[1] == n_nodes
        x, h = self.sample_from_masks(node_mask, edge_mask, context, fix_noise=fix_noise, **given(locals()))
        if self.debug_checks:
            self._check_mean_zero(x, node_mask)
        max_cog = torch.sum(x, dim=1, keepdim=True).abs().max()
        if self.debug_checks and max_cog.item() > 5e-2:
            print(f'Warning cog drift with error {max_cog.item():.3f}. Projecting the positions down.')
            nm = node_mask.to(torch.float32)
            x = x - (x.sum(1, keepdim=True) / nm.sum(1, keepdim=True)) * nm
        return x, h

    @torch.no_grad()
    def sample_chain(self, n_samples, n_nodes, node_mask, edge_mask, context, keep_frames=None, *,
                     steps=None, eta=None, spacing=None, timesteps=None, guidance_scale=None, guidance_context=None,
                     guidance_rescale=None, solver=None, lower_order_final=None, record=None, corrector=None):
        """en_diffusion.py:669-710: the reverse chain of `sample` with `keep_frames` of its states kept (None: all of them - T on
        the full chain, the number of transitions of a few-step one).  Returns [n_samples * keep_frames, N, D], frame-major, in data
        units: frame (s * keep_frames) // T holds z_s (the last state that falls into a frame stays) and frame 0 cat(x, h) of the
        decode.  The keyword-only extras are those of `sample`, plus record="x0": the data prediction instead of the state.
        Recorded inside the library's loop (`sample_from_masks`)."""
        assert node_mask.shape[0] == n_samples and node_mask.shape[1] == n_nodes
        few = given(locals())
        if keep_frames is None:                          # all of them: K of the path keywords alone (`record` needs keep_frames)
            pe = self._resolve_path(steps, eta, spacing, timesteps, solver=solver, lower_order_final=lower_order_final)
            few["keep_frames"] = self.T if pe is None else len(pe[0]) - 1
        _, _, chain = self.sample_from_masks(node_mask, edge_mask, context, **few)
        return chain.reshape(n_samples * chain.shape[0], n_nodes, chain.shape[3])
