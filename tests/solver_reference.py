"""Float64 restatement of second-order multistep sampling (DPM-Solver++ 2M; hd_set_path_multistep / hd_multistep_step), the
yardstick of tests/test_solver_cpu.py and tests/test_gpu_solver.py.  Independent of hierdiff_amd.paths: rows in Python floats
(math module), the chain on `oracle.egnn_oracle.dynamics_forward`, and the analytic Gaussian-data model whose deterministic flow
is known in closed form.

With alpha^2 = sigmoid(-gamma), sigma^2 = sigmoid(gamma), lambda = log(alpha / sigma) = -gamma / 2 and, for transition k from
t = path[k] to s = path[k + 1], h_k = lambda_s - lambda_t, r_k = h_{k-1} / h_k:
    x^_k = p z_t - q eps,                       p = 1 / alpha_t, q = sigma_t / alpha_t
    z_s  = (a z_t - b eps) + c2 (x^_k - x^_{k-1}),   a = alpha_s / alpha_t, b = a sigma_t - sigma_s,
    c2   = alpha_s (-expm1(-h_k)) / (2 r_k);  c2 = 0 at k = 0 and, with lower_order_final, at the last transition."""
import math

import torch

from oracle import egnn_oracle as orc


def _sig(v):
    return 1.0 / (1.0 + math.exp(-v))


def alpha_sigma(g):
    return math.sqrt(_sig(-g)), math.sqrt(_sig(g))


def multistep_rows(g, path, lower_order_final=True):
    """[(a, b, c2, p, q)] per transition in Python floats; `g` indexable by grid index."""
    rows, h_prev = [], None
    K = len(path) - 1
    for k, (t, s) in enumerate(zip(path[:-1], path[1:])):
        gs, gt = float(g[s]), float(g[t])
        a_s, s_s = alpha_sigma(gs)
        a_t, s_t = alpha_sigma(gt)
        h = (gt - gs) / 2.0
        c2 = 0.0
        if k > 0 and not (lower_order_final and k == K - 1):
            c2 = a_s * (-math.expm1(-h)) / (2.0 * (h_prev / h))
        rows.append((a_s / a_t, a_s * s_t / a_t - s_s, c2, 1.0 / a_t, s_t / a_t))
        h_prev = h
    return rows


def textbook_step(g, t, s, t_prev, z, x_k, x_prev):
    """DPM-Solver++(2M) as published, from the data predictions: D = (1 + 1 / (2 r)) x^_k - x^_{k-1} / (2 r) (D = x^_k without
    history), z_s = (sigma_s / sigma_t) z_t - alpha_s expm1(-h) D.  float64 tensors."""
    gs, gt = float(g[s]), float(g[t])
    a_s, s_s = alpha_sigma(gs)
    _, s_t = alpha_sigma(gt)
    h = (gt - gs) / 2.0
    D = x_k
    if x_prev is not None:
        r = ((float(g[t_prev]) - gt) / 2.0) / h
        D = (1.0 + 1.0 / (2.0 * r)) * x_k - x_prev / (2.0 * r)
    return (s_s / s_t) * z - a_s * math.expm1(-h) * D


def centre_x(v, nm):
    """x part (first three columns) mean-removed over the valid nodes; nm [B,N,1] float64."""
    return torch.cat([orc.remove_mean_with_mask(v[:, :, :3], nm), v[:, :, 3:]], dim=2)


def step_ref(row, zt, eps, x_prev, nm):
    """(x^_k, z_s) in float64 from one row: eps centred, z_s re-centred, masked entries of x^_k zero."""
    a, b, c2, p, q = row
    nm = nm.double()
    zt, ev = zt.double(), centre_x(eps.double(), nm)
    xk = (p * zt - q * ev) * nm
    zs = a * zt - b * ev
    if c2 != 0.0:
        zs = zs + c2 * (xk - x_prev.double()) * nm
    return xk, centre_x(zs, nm)


def chain_ref(eps_fn, g, path, z, nm, lower_order_final=True):
    """z_0 (float32, rounded once per transition as the device loop keeps it) of the multistep chain from the state z at path[0];
    eps_fn(z fp32, t) -> eps^ [B,N,D]."""
    rows = multistep_rows(g, path, lower_order_final)
    x_prev = None
    for k, t in enumerate(path[:-1]):
        x_prev, zs = step_ref(rows[k], z, eps_fn(z, t), x_prev, nm)
        z = zs.float()
    return z


def network_eps(sd, cfg, T, nm, em, ctx):
    """eps_fn of the EGNN oracle."""
    B, N = nm.shape[:2]

    def fn(z, t):
        t_arr = torch.full((B, 1), t, dtype=torch.int64)
        with torch.no_grad():
            return orc.dynamics_forward(sd, cfg, t_arr / T, z, nm, em, ctx, N, prefix="dynamics.egnn.")
    return fn


def guided_eps(fn_c, fn_u, w, nm):
    """eps_u + w_b (eps_c - eps_u) in float64, masked (no rescale)."""
    wv = torch.as_tensor(w, dtype=torch.float64).reshape(-1, 1, 1)
    return lambda z, t: (lambda c, u: (u + wv * (c - u)) * nm.double())(fn_c(z, t).double(), fn_u(z, t).double())


# ----------------------------------------------------------------------------- the analytic model
# Data N(0, c^2) per component: the optimal noise prediction is eps*(z, t) = sigma_t z / (alpha_t^2 c^2 + sigma_t^2), and the
# deterministic (probability-flow) solution from T to 0 is z_0 = z_T sqrt(v_0 / v_T) with v = alpha^2 c^2 + sigma^2.

def analytic_grid(T=1000):
    return [-5.0 + 15.0 * i / T for i in range(T + 1)]


def analytic_eps(g, t, z, c2data):
    a, s = alpha_sigma(float(g[t]))
    return z * (s / (a * a * c2data + s * s))


def analytic_exact(g, T, zT, c2data):
    v = lambda t: (lambda a, s: a * a * c2data + s * s)(*alpha_sigma(float(g[t])))
    return zT * math.sqrt(v(0) / v(T))


def uniform_path(T, K):
    return [T - (2 * k * T + K) // (2 * K) for k in range(K + 1)]


def analytic_run(g, path, zT, c2data, second, lower_order_final=True):
    """z_0 in float64 of the scalar (component-wise) chain without any centring: `second` False runs the eta = 0 rows."""
    rows = multistep_rows(g, path, lower_order_final)
    z, x_prev = zT.double(), None
    for k, t in enumerate(path[:-1]):
        a, b, c2, p, q = rows[k]
        ev = analytic_eps(g, t, z, c2data)
        xk = p * z - q * ev
        zs = a * z - b * ev
        if second and c2 != 0.0:
            zs = zs + c2 * (xk - x_prev)
        z, x_prev = zs, xk
    return z


def rel_err(z, ref):
    return float((z.double() - ref.double()).norm() / ref.double().norm())


def order_bounds(err2m, errdd):
    """The three properties of the convergence tests on dicts K -> error (K in {40, 80, 160}); returns the figures."""
    out = {}
    for K in (40, 80):
        out["2m", K] = err2m[K] / err2m[2 * K]
        out["ddim", K] = errdd[K] / errdd[2 * K]
    return out
