"""CPU restatement of the editing entry points (DiffusionQM9.diffuse / encode / sample_from_latent / slerp; algorithm in
include/hierdiff_hip.h, "Editing given molecules"), the yardstick of tests/test_edit_cpu.py and tests/test_gpu_edit.py.

Built from the oracle's own pieces the way `path_chain_ref` of tests/test_gpu_fewstep.py is: `oracle.egnn_oracle.dynamics_forward`
for the network, `posterior_step` for ancestral transitions, `final_decode`, `combined_noise`, `remove_mean_with_mask`.  The
coefficient rows are evaluated here with Python floats (math module), independent of hierdiff_amd.paths.

`RefNet(..., dtype=torch.float64)` evaluates the same formulas in double precision throughout (`oracle.egnn_oracle.float64`): the
yardstick for "is the parity bar passable by correct fp32 arithmetic" (test_edit_cpu.py, section 8).  In the default float32 form the
rows are float64 and the state is rounded to fp32 once per transition, as the device loop keeps it.
"""
import math

import numpy as np
import torch

from oracle import egnn_oracle as orc

SLERP_EPS = 1e-6            # documented at hd_slerp: below this sin(theta) the linear form is used


# ----------------------------------------------------------------------------- rows (Python floats)

def _sig(v):
    return 1.0 / (1.0 + math.exp(-v))


def alpha_sigma(g):
    """(alpha, sigma) of a gamma value in Python floats."""
    return math.sqrt(_sig(-g)), math.sqrt(_sig(g))


def up_row(gu, gv):
    """(a, b) of z_v = a z_u - b eps for u < v."""
    a_u, s_u = alpha_sigma(gu)
    a_v, s_v = alpha_sigma(gv)
    return a_v / a_u, a_v / a_u * s_u - s_v


def down_row(gs, gt, eta):
    """(a, b, c) of z_s = a z_t - b eps + c noise for s < t (the DDIM family; eta = 0: noise-free)."""
    softplus = lambda v: max(v, 0.0) + math.log1p(math.exp(-abs(v)))
    a_s, s_s = alpha_sigma(gs)
    a_t, s_t = alpha_sigma(gt)
    st = eta * math.sqrt(-math.expm1(softplus(gs) - softplus(gt))) * s_s / s_t
    return a_s / a_t, a_s * s_t / a_t - math.sqrt(max(s_s * s_s - st * st, 0.0)), st


# ----------------------------------------------------------------------------- the network and the oracle's steps

class RefNet:
    """The oracle's network for one batch (masks, context) on a T-step grid; dtype float32 (default) or float64."""

    def __init__(self, sd_np, cfg, T, node_mask, edge_mask, context=None, dtype=torch.float32):
        self.cfg, self.T, self.dtype = cfg, int(T), dtype
        self.nm, self.em, self.ctx = node_mask, edge_mask, context
        self.B, self.N = node_mask.shape[:2]
        with self:
            self.sd = orc.as_torch_sd(sd_np)

    def __enter__(self):
        if self.dtype == torch.float64:
            self._f64 = orc.float64()
            self._f64.__enter__()

    def __exit__(self, *exc):
        if self.dtype == torch.float64:
            self._f64.__exit__(*exc)

    def _time(self, idx):
        return torch.full((self.B, 1), int(idx), dtype=torch.int64) / self.T

    def net(self, z, t_idx):
        """eps^ [B,N,D] at the grid index t_idx."""
        with self, torch.no_grad():
            return orc.dynamics_forward(self.sd, self.cfg, self._time(t_idx), z, self.nm, self.em, self.ctx, self.N,
                                        prefix="dynamics.egnn.")

    def post(self, z, s, t, raw, gg):
        """The ancestral transition t -> s."""
        with self, torch.no_grad():
            return orc.posterior_step(self.sd, self.cfg, self._time(s), self._time(t), z, self.nm, self.em, self.ctx, raw,
                                      mol_shape=self.N, gammas=(gg[s].expand(self.B, 1), gg[t].expand(self.B, 1)))

    def decode(self, z, raw, gg):
        with self, torch.no_grad():
            return orc.final_decode(self.sd, self.cfg, z, self.nm, self.em, self.ctx, raw, gamma_0=gg[0].expand(self.B, 1))


class FixedEps:
    """Network stand-in that returns the same eps whatever z and t (tests of the host arithmetic alone)."""

    def __init__(self, eps, node_mask, dtype=torch.float32):
        self.eps, self.nm, self.dtype = eps, node_mask, dtype

    def net(self, z, t_idx):
        return self.eps.clone()


def _centre_x(v, nmf):
    return torch.cat([orc.remove_mean_with_mask(v[:, :, :3], nmf), v[:, :, 3:]], dim=2)


# ----------------------------------------------------------------------------- the four restatements

def normalised_data(x, h, node_mask, dtype=torch.float32):
    """xh [B,N,D] of raw (x, h) under the unit normalisation the tests' models use: x re-centred per molecule, h masked."""
    nmf = node_mask.to(dtype)
    x = orc.remove_mean_with_mask(x.to(dtype) * nmf, nmf)
    return torch.cat([x, h.to(dtype) * nmf], dim=2)


def diffuse_ref(x, h, node_mask, g_t, raw, dtype=torch.float32):
    """z_t = alpha_t xh + sigma_t eps; raw = (randn_x [b,N,3], randn_h [b,N,F]), b = 1: one row shared by the batch.  alpha / sigma
    are the fp32 values the product passes to hd_diffuse (float64 form: Python floats of the same gamma)."""
    nmf = node_mask.to(dtype)
    xh = normalised_data(x, h, node_mask, dtype)
    eps = orc.combined_noise(raw[0].to(dtype), raw[1].to(dtype), nmf)
    if dtype == torch.float32:
        g = torch.as_tensor(g_t, dtype=torch.float32)
        alpha, sigma = torch.sqrt(torch.sigmoid(-g)), torch.sqrt(torch.sigmoid(g))
    else:
        alpha, sigma = alpha_sigma(float(g_t))
    return alpha * xh + sigma * eps


def encode_ref(net, gg, path_up, xh, node_mask):
    """z at path_up[-1] from z_0 = alpha_0 xh by the noise-free update run upwards over `path_up` (ascending grid indices from 0).
    float64 rows; the state is kept in net.dtype (fp32: rounded once per transition)."""
    dt = net.dtype
    nmd = node_mask.to(torch.float64)
    if dt == torch.float32:
        z = torch.sqrt(torch.sigmoid(-torch.as_tensor(gg[0], dtype=torch.float32))) * xh.to(dt)
    else:
        z = alpha_sigma(float(gg[0]))[0] * xh.to(dt)
    for u, v in zip(path_up[:-1], path_up[1:]):
        a, b = up_row(float(gg[u]), float(gg[v]))
        eps = _centre_x(net.net(z, u).double(), nmd)
        z = _centre_x(a * z.double() - b * eps, nmd).to(dt)
    return z


def partial_chain_ref(net, gg, path, eta, z, node_mask, raws, decode=True):
    """The reverse chain on the descending `path` (path[0] = the grid index of z, path[-1] = 0) from a given state, with injected
    normals raws = [one pair per transition (, the decode)].  eta = 1: the oracle's posterior_step; eta < 1: the float64 formula on
    the oracle's network, as path_chain_ref of tests/test_gpu_fewstep.py.  Returns (x, h, z_0), or z_0 alone with decode=False."""
    dt = net.dtype
    nmf = node_mask.to(dt)
    nmd = node_mask.to(torch.float64)
    z = z.to(dt)
    for k, (t, s) in enumerate(zip(path[:-1], path[1:])):
        if eta == 1.0:
            z = net.post(z, s, t, raws[k], gg)
            continue
        a, b, c = down_row(float(gg[s]), float(gg[t]), eta)
        eps = _centre_x(net.net(z, t).double(), nmd)
        zs = a * z.double() - b * eps
        if c != 0.0:
            zs = zs + c * orc.combined_noise(raws[k][0], raws[k][1], nmf).double()
        z = _centre_x(zs, nmd).to(dt)
    if not decode:
        return z
    x, h = net.decode(z, raws[len(path) - 1], gg)
    return x, h, z


def slerp_ref(za, zb, lambdas, node_mask):
    """[L,B,N,D] float64 (numpy): per molecule theta = acos(clamp(<a, b> / (|a| |b|))) over the valid entries and
    (sin((1 - lam) theta) a + sin(lam theta) b) / sin theta; the linear form where sin theta < SLERP_EPS or a latent is zero;
    lam = 0 / 1 return a / b; masked entries 0."""
    a = np.asarray(za, dtype=np.float64)
    b = np.asarray(zb, dtype=np.float64)
    m = np.asarray(node_mask, dtype=np.float64).reshape(a.shape[0], a.shape[1], 1)
    a, b = a * m, b * m
    out = np.zeros((len(lambdas),) + a.shape)
    for i in range(a.shape[0]):
        na, nb = math.sqrt(float((a[i] * a[i]).sum())), math.sqrt(float((b[i] * b[i]).sum()))
        theta = st = 0.0
        if na * nb > 0.0:
            theta = math.acos(min(1.0, max(-1.0, float((a[i] * b[i]).sum()) / (na * nb))))
            st = math.sin(theta)
        for l, lam in enumerate(lambdas):
            lam = float(lam)
            if lam == 0.0:
                out[l, i] = a[i]
            elif lam == 1.0:
                out[l, i] = b[i]
            elif st < SLERP_EPS:
                out[l, i] = (1.0 - lam) * a[i] + lam * b[i]
            else:
                out[l, i] = (math.sin((1.0 - lam) * theta) * a[i] + math.sin(lam * theta) * b[i]) / st
    return out


# ----------------------------------------------------------------------------- the shared cases

MAIN = dict(T=20, H=32, L=2, n_list=[7, 4, 1])         # the one-node molecule: x noise exactly 0 after the mean removal
WRAP = dict(T=20, H=32, L=2, n_list=[30, 17])          # N * D = 330 > 256: the strided loops of k_diffuse / k_slerp wrap
WEIGHT_SEED = 31


def weights(H, L, C_=0, seed=WEIGHT_SEED):
    """(sd_np, oracle cfg) of the synthetic weights the trajectory tests use (coordinate gain 0.02: an O(1) velocity)."""
    from hierdiff_amd.weights import synthetic_state_dict
    sd_np = synthetic_state_dict(9, C_, H, L, 2, True, seed, 0.02)
    return sd_np, orc.DynCfg(in_node_nf=9, context_node_nf=C_, hidden_nf=H, n_layers=L)


def cpu_diffusion(sd_np, H, L, T, C_=0):
    from hierdiff_amd import DiffusionQM9, default_config
    m = DiffusionQM9(default_config(hidden_nf=H, n_layers=L, context_node_nf=C_, timesteps=T))
    m.load_state_dict({k: torch.from_numpy(np.asarray(v).copy()) for k, v in sd_np.items()})
    return m


def molecules(n_list, seed=5, C_=0):
    """(x, h, node_mask bool [B,N,1], edge_mask, context or None): seeded raw data on the canonical masks."""
    nm, em = orc.canonical_masks(n_list)
    B, N = nm.shape[:2]
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, N, 3, generator=g) * nm
    h = torch.randn(B, N, 8, generator=g) * nm
    ctx = None
    if C_:
        ctx = torch.randn(B, 1, 1, generator=g).expand(B, N, 1).contiguous() * nm.float()
    return x, h, nm.bool(), em, ctx


def raw_draws(n, B, N, seed, rows=None):
    g = torch.Generator().manual_seed(seed)
    b = B if rows is None else rows
    return [(torch.randn(b, N, 3, generator=g), torch.randn(b, N, 8, generator=g)) for _ in range(n)]
