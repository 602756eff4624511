"""Float64 restatement of stochastic second-order multistep sampling (SDE-DPM-Solver++ 2M; hd_set_path_multistep_sde /
hd_multistep_sde_step), the yardstick of tests/test_sde_solver_cpu.py and tests/test_gpu_sde_solver.py.  Independent of
hierdiff_amd.paths: rows in Python floats (math module) FROM THE PUBLISHED FORM, the chain on `oracle.egnn_oracle.dynamics_forward`,
and the exact variance recursion of the analytic Gaussian-data model.

With alpha^2 = sigmoid(-gamma), sigma^2 = sigmoid(gamma), lambda = log(alpha / sigma) = -gamma / 2 and, for transition k from
t = path[k] to s = path[k + 1], h = lambda_s - lambda_t, r = h_{k-1} / h_k, the update as published is
    z_s = (sigma_s / sigma_t) e^{-h} z_t + alpha_s (1 - e^{-2h}) x^_k + 1/2 alpha_s (1 - e^{-2h}) (x^_k - x^_{k-1}) / r
          + sigma_s sqrt(1 - e^{-2h}) xi,        x^_k = (z_t - sigma_t eps) / alpha_t.
Collecting z_t and eps (x^_k = p z_t - q eps, p = 1 / alpha_t, q = sigma_t / alpha_t) gives the row the library runs,
    z_s = ((a z_t - b eps) + c xi) + c2 (x^_k - x^_{k-1}),
    a = (sigma_s / sigma_t) e^{-h} + alpha_s (1 - e^{-2h}) p,   b = alpha_s (1 - e^{-2h}) q,   c = sigma_s sqrt(1 - e^{-2h}),
    c2 = alpha_s (1 - e^{-2h}) / (2 r);  c2 = 0 at k = 0 and, with lower_order_final, at the last transition."""
import math

import numpy as np
import torch

from oracle import egnn_oracle as orc
from tests import solver_reference as sr

alpha_sigma = sr.alpha_sigma
centre_x = sr.centre_x
network_eps = sr.network_eps
guided_eps = sr.guided_eps
analytic_grid = sr.analytic_grid
uniform_path = sr.uniform_path


def published_coefficients(gs, gt):
    """(A, Bx, C) of z_s = A z_t + Bx x^_k + (Bx / (2 r)) (x^_k - x^_{k-1}) + C xi, and h; Python floats."""
    a_s, s_s = alpha_sigma(gs)
    _, s_t = alpha_sigma(gt)
    h = (gt - gs) / 2.0
    one_m = -math.expm1(-2.0 * h)                      # 1 - e^{-2h}
    return (s_s / s_t) * math.exp(-h), a_s * one_m, s_s * math.sqrt(one_m), h


def sde_rows(g, path, lower_order_final=True):
    """[(a, b, c, c2, p, q)] per transition in Python floats; `g` indexable by grid index."""
    rows, h_prev = [], None
    K = len(path) - 1
    for k, (t, s) in enumerate(zip(path[:-1], path[1:])):
        gs, gt = float(g[s]), float(g[t])
        A, Bx, Cn, h = published_coefficients(gs, gt)
        a_t, s_t = alpha_sigma(gt)
        p, q = 1.0 / a_t, s_t / a_t
        c2 = 0.0
        if k > 0 and not (lower_order_final and k == K - 1):
            c2 = 0.5 * Bx / (h_prev / h)
        rows.append((A + Bx * p, Bx * q, Cn, c2, p, q))
        h_prev = h
    return rows


def ancestral_rows(g, path):
    """The first-order member of the family: the same rows with every c2 = 0 (ancestral sampling, eta = 1)."""
    return [(a, b, c, 0.0, p, q) for (a, b, c, _, p, q) in sde_rows(g, path, True)]


def published_step(g, t, s, t_prev, z, x_k, x_prev, xi):
    """The update as published, from the data predictions; float64 tensors.  x_prev None: no history (first order)."""
    gs, gt = float(g[s]), float(g[t])
    A, Bx, Cn, h = published_coefficients(gs, gt)
    out = A * z + Bx * x_k + Cn * xi
    if x_prev is not None:
        r = ((float(g[t_prev]) - gt) / 2.0) / h
        out = out + 0.5 * Bx * (x_k - x_prev) / r
    return out


def folded_step(row, z, eps, x_prev, xi):
    """(x^_k, z_s) of the row the library runs, no centring; float64 tensors."""
    a, b, c, c2, p, q = row
    xk = p * z - q * eps
    zs = (a * z - b * eps) + c * xi
    if c2 != 0.0:
        zs = zs + c2 * (xk - x_prev)
    return xk, zs


def _mean_abs(v, nm):
    return (v * nm).sum(1, keepdim=True) / nm.sum(1, keepdim=True) * nm


def step_ref(row, zt, eps, x_prev, nm, raw, mol=None, magnitudes=False):
    """(x^_k, z_s) in float64 on the first `mol` nodes from one row: eps and the noise (raw = (randn_x [rows,mol,3], randn_h
    [rows,mol,F])) centred and masked, z_s re-centred, masked entries of x^_k zero.  With `magnitudes` also (A_x, A_z): the same
    formulas with every term replaced by its absolute value and every mean by the mean of the absolute values (the magnitude
    arrays of tests/sampling_reference.py)."""
    a, b, c, c2, p, q = row
    N = zt.shape[1]
    mol = N if mol is None else mol
    nm = nm.double().reshape(zt.shape[0], N, 1)[:, :mol]
    zt, ev_raw = zt.double()[:, :mol], eps.double()[:, :mol]
    B = zt.shape[0]
    ev = centre_x(ev_raw, nm)
    rx, rh = raw[0].double().expand(B, -1, -1), raw[1].double().expand(B, -1, -1)
    xi_raw = torch.cat([rx, rh], dim=2) * nm
    xi = centre_x(xi_raw, nm)
    xk = (p * zt - q * ev) * nm
    zs = (a * zt - b * ev) + c * xi
    if c2 != 0.0:
        zs = zs + c2 * (xk - x_prev.double()[:, :mol]) * nm
    out = centre_x(zs, nm)
    if not magnitudes:
        return xk, out

    def with_mean(v):
        return torch.cat([v[:, :, :3] + _mean_abs(v[:, :, :3], nm), v[:, :, 3:]], dim=2)
    a_ev, a_xi = with_mean(ev_raw.abs()), with_mean(xi_raw.abs())
    A_x = (abs(p) * zt.abs() + abs(q) * a_ev)
    A_v = abs(a) * zt.abs() + abs(b) * a_ev + abs(c) * a_xi
    if c2 != 0.0:
        A_v = A_v + abs(c2) * (A_x + x_prev.double()[:, :mol].abs()) * nm
    return xk, out, A_x, with_mean(A_v)


def chain_ref(eps_fn, g, path, z, nm, raws, lower_order_final=True, rows=None):
    """[(z_s float32, x^_k float64)] per transition of the chain from the state z at path[0]: every state rounded once to float32
    as the device loop keeps it.  eps_fn(z fp32, t) -> eps^ [B,N,D]; raws[k] = (randn_x, randn_h) of transition k."""
    rows = sde_rows(g, path, lower_order_final) if rows is None else rows
    x_prev, out = None, []
    for k, t in enumerate(path[:-1]):
        x_prev, zs = step_ref(rows[k], z, eps_fn(z, t), x_prev, nm, raws[k])
        z = zs.float()
        out.append((z, x_prev))
    return out


def steered_chain_ref(inner, rs, gg, path, beta, P, rho, seed, base, T, F, z, lower_order_final=False, gather_history=True):
    """(states, x^ per transition, infos, final steering State) of the steered sde2m chain over `inner` (.net(z, t), .nm: a RefNet or
    a RestrainedNet): the stage of tests/steer_reference.py behind every network call, then the update above with the generator's
    own normals (host twins).  The history x^_{k-1} travels with the lineage: rows that receive another row's z_t and eps^ receive
    its x^_{k-1} too.  `gather_history=False` is the WRONG chain that leaves the history in its row."""
    from tests import steer_reference as st
    nm = inner.nm
    B, N = nm.shape[:2]
    rows = sde_rows(gg, path, lower_order_final)
    srows = st.steer_rows(gg, path, beta)
    state = st.State(B, P)
    x_prev, states, xs, infos = None, [], [], []
    for k, (t, s) in enumerate(zip(path[:-1], path[1:])):
        eps = inner.net(z, t)
        draw = T - s
        z, eps, info = st.stage(rs, z, eps, nm, srows[k], 1.0, state, rho, seed, base, draw)
        if x_prev is not None and gather_history:
            x_prev = x_prev[torch.from_numpy(info["anc"])]
        raw = st.normals_host(seed, base, draw, B, N, F)
        x_prev, zs = step_ref(rows[k], z, eps, x_prev, nm.float(), raw)
        z = zs.float()
        states.append(z)
        xs.append(x_prev)
        infos.append(info)
    return states, xs, infos, state


# ----------------------------------------------------------------------------- the analytic model: the exact variance recursion
# Data N(0, c^2) per component: eps*(z, t) = kappa_t z with kappa_t = sigma_t / (alpha_t^2 c^2 + sigma_t^2).  The sampler is linear in
# u = (z_k, x^_{k-1}) and xi: x^_k = m_k z_k with m_k = p - q kappa, and
#     z_{k+1} = (a - b kappa + c2 m_k) z_k - c2 x^_{k-1} + c xi,
# so Cov(u) follows Cov' = M Cov M^T + diag(c^2, 0) with M = [[a - b kappa + c2 m_k, -c2], [m_k, 0]], from Cov = diag(1, 0) (the
# sampler starts from a standard normal).  The exact marginal is Var(z_0) = alpha_0^2 c^2 + sigma_0^2.  No sampling noise enters.

def variance_z0(rows, g, path, c2data=1.0):
    v11, v12, v22 = 1.0, 0.0, 0.0
    for k, t in enumerate(path[:-1]):
        a, b, c, c2, p, q = (float(v) for v in rows[k])
        a_t, s_t = alpha_sigma(float(g[t]))
        kappa = s_t / (a_t * a_t * c2data + s_t * s_t)
        m = p - q * kappa
        f = a - b * kappa + c2 * m
        # M = [[f, -c2], [m, 0]]
        n11 = f * f * v11 - 2.0 * f * c2 * v12 + c2 * c2 * v22 + c * c
        n12 = m * (f * v11 - c2 * v12)
        n22 = m * m * v11
        v11, v12, v22 = n11, n12, n22
    return v11


def variance_error(rows, g, path, c2data=1.0):
    """|Var(z_0) of the sampler - exact| / exact."""
    a0, s0 = alpha_sigma(float(g[path[-1]]))
    exact = a0 * a0 * c2data + s0 * s0
    return abs(variance_z0(rows, g, path, c2data) - exact) / exact


def rel_l2_t(got, ref):
    return float((got.double() - ref.double()).norm() / ref.double().norm())


def ratio(got, ref, A, nm):
    """(worst |err| / (2^-23 A) over the valid elements, number of masked elements that are not exactly 0): numpy arrays."""
    valid = np.broadcast_to(np.asarray(nm).reshape(ref.shape[0], -1)[:, :ref.shape[1], None] != 0, ref.shape)
    err = np.abs(np.asarray(got, np.float64) - ref)
    assert np.all(A[valid] > 0)
    return float(np.max(err[valid] / (2.0 ** -23 * A[valid]))), int(np.count_nonzero(np.asarray(got)[~valid]))
