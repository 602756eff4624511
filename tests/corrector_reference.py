"""Float64 restatement of predictor-corrector sampling (hd_langevin_step / the corrected path loop; formulas in
include/hierdiff_hip.h, "Predictor-corrector sampling"), the yardstick of tests/test_corrector_cpu.py and tests/test_gpu_corrector.py.

`langevin_ref` is the step in numpy float64, written from the formulas; it returns the value together with a MAGNITUDE array `A` (the
same formula with every term replaced by its absolute value and every mean by the mean of the absolute values over the valid nodes,
as tests/sampling_reference.py builds it) and the gains.  A correct float32 evaluation stays within BOUND * U * A = 8 * 2^-23 * A
element by element: the step is the posterior step's expression with two coefficients that were rounded once (one more rounding each,
inside the 4 + 12 of the derivation there), and the gain is a double.  `langevin_f32` is the float32 twin with a `mutant=` switch:
the wrong kernels the bar has to reject.  `corrected_chain` runs C corrector steps ahead of every predictor step of a chain over any
eps function (the oracle's network, wrapped by the restatements of the loop terms), with the generator's normals from its host twin
at the draws of the layout: stream 0 for the predictor, stream 1 + c for corrector step c, `stride = T + 2` draws apart.

Nothing is imported from the product but the host twin of the counter-based generator, which is tested on its own."""
import math

import numpy as np
import torch

U = 2.0 ** -23
BOUND = 8.0
MUTANTS = ("xi_mean_kept", "norms_over_masked", "sqrt_g", "cap_ignored", "sigma_dropped", "stream_c")


# ----------------------------------------------------------------------------- rows

def _softplus(v):
    return max(v, 0.0) + math.log1p(math.exp(-abs(v)))


def rows_from_grid(g, path, mode, strength, max_gain=math.inf):
    """[K, 3] float32 rows {sigma_t, q_k, g_max_k}: q_k = 2 r_k^2 alpha^2_{t|s} (mode "snr", strength = r) or the gain itself
    (mode "fixed"); Python floats, rounded once.  `g` indexable by grid index."""
    K = len(path) - 1
    st = list(strength) if isinstance(strength, (list, tuple)) else [strength] * K
    out = np.empty((K, 3), dtype=np.float32)
    for k, (t, s) in enumerate(zip(path[:-1], path[1:])):
        gt, gs = float(g[t]), float(g[s])
        sigma_t = math.sqrt(1.0 / (1.0 + math.exp(-gt)))
        alpha2_ts = math.exp(_softplus(gs) - _softplus(gt))
        out[k] = (sigma_t, st[k] if mode == "fixed" else 2.0 * st[k] * st[k] * alpha2_ts, max_gain)
    return out


# ----------------------------------------------------------------------------- the step

def _centre(v, m, cnt):
    """x columns freed of their mean over the valid nodes; v already masked.  [N, D] arrays, m [N, 1]."""
    out = v.copy()
    out[:, :3] -= (v[:, :3].sum(0, keepdims=True) / cnt) * m
    return out


def _abs_centre(v, m, cnt):
    a = np.abs(v)
    a[:, :3] += (a[:, :3].sum(0, keepdims=True) / cnt) * m
    return a


def langevin_ref(z, eps, nm, row3, adaptive, raw_x, raw_h):
    """(z' [B,N,D] float64 - masked rows hold z -, A, gains [B], kept [B] bool).  z, eps [B,N,D]; nm [B,N]; row3 {sigma_t, q, g_max}
    as float32; raw_x [rows,N,3], raw_h [rows,N,F] with rows 1 (shared) or B.  A kept molecule returns z itself, gain 0."""
    z64, e64 = np.asarray(z, np.float64), np.asarray(eps, np.float64)
    nm = np.asarray(nm) != 0
    B, N, D = z64.shape
    sigma_t, q, gmax = (float(np.float32(v)) for v in row3)
    out, A = z64.copy(), np.abs(z64)
    gains, kept = np.zeros(B), np.ones(B, dtype=bool)
    if q == 0.0:
        return out, A, gains, kept
    raw = np.concatenate([np.asarray(raw_x, np.float64), np.asarray(raw_h, np.float64)], axis=2)
    for b in range(B):
        m = nm[b].astype(np.float64)[:, None]
        cnt = m.sum()
        if cnt == 0:
            continue
        with np.errstate(invalid="ignore", over="ignore"):
            ev_raw = np.where(m != 0, e64[b], 0.0)
            xi_raw = raw[0 if raw.shape[0] == 1 else b] * m
            ev, xi = _centre(ev_raw, m, cnt), _centre(xi_raw, m, cnt)
            n_xi, n_eps = float((xi * xi * m).sum()), float((ev * ev * m).sum())
        if not (n_eps > 0.0 and math.isfinite(n_xi) and math.isfinite(n_eps)):
            continue
        g = q
        if adaptive:
            g = min(gmax, q * n_xi / n_eps)
        if g == 0.0 or not math.isfinite(g):
            continue
        c_eps, c_xi = float(np.float32(g * sigma_t)), float(np.float32(sigma_t * math.sqrt(2.0 * g)))
        v = (z64[b] - c_eps * ev) + c_xi * xi
        a = np.abs(z64[b]) + c_eps * _abs_centre(ev_raw, m, cnt) + c_xi * _abs_centre(xi_raw, m, cnt)
        a[:, :3] += (a[:, :3] * m).sum(0, keepdims=True) / cnt * m
        v[:, :3] -= (v[:, :3] * m).sum(0, keepdims=True) / cnt * m
        valid = nm[b]
        out[b][valid], A[b][valid] = v[valid], a[valid]
        gains[b], kept[b] = g, False
    return out, A, gains, kept


f32 = np.float32


def langevin_f32(z, eps, nm, row3, adaptive, raw_x, raw_h, mutant=None):
    """The float32 twin of `langevin_ref` (what a correct kernel computes, up to the order of its sums; the norms and the gain in
    double as the kernel keeps them), or with `mutant` one of MUTANTS[:5] a wrong one ("stream_c" is a mutant of the chain).
    Returns (z' float32, gains)."""
    assert mutant is None or mutant in MUTANTS
    z32, e32 = np.asarray(z, f32), np.asarray(eps, f32)
    nm = np.asarray(nm) != 0
    B, N, D = z32.shape
    sigma_t, q, gmax = (f32(v) for v in row3)
    out, gains = z32.copy(), np.zeros(B)
    if q == 0:
        return out, gains
    raw = np.concatenate([np.asarray(raw_x, f32), np.asarray(raw_h, f32)], axis=2)
    for b in range(B):
        m = nm[b].astype(f32)[:, None]
        cnt = m.sum(dtype=f32)
        if cnt == 0:
            continue
        with np.errstate(invalid="ignore", over="ignore"):
            ev = np.where(m != 0, e32[b], f32(0))
            xi = raw[0 if raw.shape[0] == 1 else b] * m
            ev[:, :3] -= (ev[:, :3].sum(0, keepdims=True, dtype=f32) / cnt) * m
            if mutant != "xi_mean_kept":
                xi[:, :3] -= (xi[:, :3].sum(0, keepdims=True, dtype=f32) / cnt) * m
            if mutant == "norms_over_masked":                 # the raw arrays, masked rows included
                full_e = e32[b].astype(np.float64)
                full_x = raw[0 if raw.shape[0] == 1 else b].astype(np.float64)
                n_xi, n_eps = float((full_x * full_x).sum()), float((full_e * full_e).sum())
            else:
                n_xi = float((xi.astype(np.float64) ** 2 * m).sum())
                n_eps = float((ev.astype(np.float64) ** 2 * m).sum())
        if not (n_eps > 0.0 and math.isfinite(n_xi) and math.isfinite(n_eps)):
            continue
        g = float(q)
        if adaptive:
            g = float(q) * n_xi / n_eps
            if mutant != "cap_ignored":
                g = min(float(gmax), g)
        if g == 0.0 or not math.isfinite(g):
            continue
        c_eps = f32(g) if mutant == "sigma_dropped" else f32(g * float(sigma_t))
        c_xi = f32(float(sigma_t) * math.sqrt(g if mutant == "sqrt_g" else 2.0 * g))
        v = ((z32[b] - c_eps * ev) + c_xi * xi).astype(f32)
        v[:, :3] -= ((v[:, :3] * m).sum(0, keepdims=True, dtype=f32) / cnt) * m
        out[b][nm[b]] = v[nm[b]]
        gains[b] = g
    return out, gains


def gain_slack(nm, raw_x, raw_h, delta):
    """[B]: how far the gain of mode "snr" can move, relatively, when every normal moves by at most `delta`: d(n_xi^2) / n_xi^2 <=
    2 delta sum |xi~| / sum xi~^2 (the mean removal is a projection: it does not enlarge the perturbation's 2-norm, and
    sum |xi~| |d| <= delta sum |xi~| bounds the cross term; the quadratic term is below it for delta << |xi~|)."""
    nm = np.asarray(nm) != 0
    raw = np.concatenate([np.asarray(raw_x, np.float64), np.asarray(raw_h, np.float64)], axis=2)
    out = np.zeros(nm.shape[0])
    for b in range(nm.shape[0]):
        m = nm[b].astype(np.float64)[:, None]
        if m.sum() == 0:
            continue
        xi = _centre(raw[0 if raw.shape[0] == 1 else b] * m, m, m.sum())
        if (xi * xi).sum() > 0:
            out[b] = 2.0 * delta * (np.abs(xi).sum() + delta * xi.size) / (xi * xi).sum()
    return out


def ratio(got, ref, A, nm):
    """Worst |err| / (U * A) over the valid elements."""
    valid = np.broadcast_to((np.asarray(nm) != 0)[:, :, None], ref.shape)
    if not valid.any():
        return 0.0
    err = np.abs(np.asarray(got, np.float64) - ref)
    assert np.all(A[valid] > 0)
    return float(np.max(err[valid] / (U * A[valid])))


# ----------------------------------------------------------------------------- the kernel cases

def kernel_case(N, D, seed=0):
    """B = 5: an ordinary molecule, one valid node, no valid node, eps^ == 0, a NaN element in eps^ - the last three keep their bits.
    z carries a centre-of-mass offset (the re-centring counts) and junk in its masked rows (they are never written)."""
    rng = np.random.Generator(np.random.PCG64([20261021, N, D, seed]))
    B, F = 5, D - 3
    nm = np.zeros((B, N), dtype=np.uint8)
    nm[0, :N - 1] = 1
    nm[0, 0], nm[0, N - 1] = 0, 1                              # not a prefix
    nm[1, N // 2] = 1
    nm[3, :] = 1
    nm[4, :max(2, N - 2)] = 1
    m = nm.astype(np.float32)[:, :, None]
    z = rng.standard_normal((B, N, D)).astype(np.float32)
    z[:, :, :3] += np.array([3.0, -2.0, 1.0], dtype=np.float32) * m
    eps = (rng.standard_normal((B, N, D)) * 1.5).astype(np.float32) * m
    eps[3] = 0.0
    eps[4, 1, D - 1] = np.nan
    c = dict(B=B, N=N, D=D, F=F, nm=nm, z=z, eps=eps,
             raw_x=rng.standard_normal((B, N, 3)).astype(np.float32), raw_h=rng.standard_normal((B, N, F)).astype(np.float32))
    c["keeps"] = np.array([False, False, True, True, True])
    return c


def kernel_rows():
    """(name, row3, adaptive): both modes, the cap active and inactive, q = 0.  With |xi~|^2 / |eps~|^2 about 1 / 2.25 the gain of
    mode "snr" at q = 0.05 is about 0.02: a cap of 0.004 binds, inf does not."""
    return [("snr", (0.7, 0.05, math.inf), 1), ("snr capped", (0.7, 0.05, 0.004), 1), ("fixed", (0.7, 0.03, math.inf), 0),
            ("fixed, cap ignored", (0.7, 0.03, 0.004), 0), ("q = 0", (0.7, 0.0, math.inf), 1), ("sigma = 0", (0.0, 0.05, math.inf), 0)]


# ----------------------------------------------------------------------------- chains

def normals_host(seed, base, draw, B, N, F, rows=None):
    """(randn_x [rows,N,3], randn_h [rows,N,F]) of the samples base .. at `draw` from the library's host twin of the generator (entry
    n * (3 + F) + c of sample base + b); rows = 1: the shared row of fix_noise."""
    from hierdiff_amd import _lib
    fn = _lib.load().hd_philox_normal_host
    D = 3 + F
    R = B if rows is None else rows
    out = np.empty((R, N, D), dtype=np.float32)
    for b in range(R):
        for e in range(N * D):
            out[b, e // D, e % D] = fn(int(seed), int(base) + b, int(draw), e)
    t = torch.from_numpy(out)
    return t[:, :, :3].contiguous(), t[:, :, 3:].contiguous()


class Draws:
    """The generator's normals of a chain on a T-step grid: `at(stream, s)` is the pair at draw (T + 2) stream + (T - s)."""

    def __init__(self, seed, base, T, B, N, F, rows=None, mutant=None):
        self.a = (seed, base), (B, N, F, rows)
        self.T, self.mutant, self.memo = int(T), mutant, {}

    def at(self, stream, s):
        d = (self.T + 2) * stream + (self.T - int(s))
        if d not in self.memo:
            (seed, base), (B, N, F, rows) = self.a
            self.memo[d] = normals_host(seed, base, d, B, N, F, rows)
        return self.memo[d]

    def corrector(self, c, s):
        return self.at(c if self.mutant == "stream_c" else 1 + c, s)


def corrector_block(z, eps_fn, t, s, nm, row3, adaptive, C, draws, step=langevin_ref):
    """C Langevin steps on z (fp32 tensor) at level t of the transition t -> s; every state rounded once to fp32, as the device loop
    keeps it.  Returns (z, gains [C, B])."""
    gains = []
    nmn = nm.reshape(z.shape[0], -1).numpy()
    for c in range(C):
        eps = eps_fn(z, t)
        rx, rh = draws.corrector(c, s)
        out = step(z.numpy(), eps.numpy(), nmn, row3, adaptive, rx.numpy(), rh.numpy())
        z = torch.from_numpy(np.asarray(out[0], dtype=np.float32))
        gains.append(out[-2] if step is langevin_ref else out[1])
    return z, np.asarray(gains)


def corrected_chain(eps_fn, predictor, path, z, nm, rows3, adaptive, C, draws, step=langevin_ref):
    """[(state after the correctors, state after the predictor)] per transition.  `predictor(k, z, eps, raw)` -> z_s (any dtype; it is
    rounded to fp32 here) is the update of transition k on eps^ with the stream-0 normals `raw`."""
    out = []
    for k, (t, s) in enumerate(zip(path[:-1], path[1:])):
        zc, _ = corrector_block(z, eps_fn, t, s, nm, rows3[k], adaptive, C, draws, step)
        z = predictor(k, zc, eps_fn(zc, t), draws.at(0, s)).float()
        out.append((zc, z))
    return out


# ----------------------------------------------------------------------------- the analytic check: Gaussian data, exact score

def gaussian_eps(z, alpha, sigma, v):
    """eps^ of the exact score of data N(0, v) at the level (alpha, sigma): the marginal is N(0, s2), s2 = alpha^2 v + sigma^2,
    score = -z / s2, eps^ = -sigma score."""
    return sigma * z / (alpha * alpha * v + sigma * sigma)


def variance_step(var, g, sigma, s2):
    """var' = (1 - g sigma^2 / s2)^2 var + 2 g sigma^2: one fixed-gain Langevin step on the Gaussian above."""
    return (1.0 - g * sigma * sigma / s2) ** 2 * var + 2.0 * g * sigma * sigma


def variance_fixed_point(g, sigma, s2):
    return s2 / (1.0 - g * sigma * sigma / (2.0 * s2))
