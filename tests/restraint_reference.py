"""Float64 restatement of restraint-guided sampling (hd_restrain_eps / hd_restraint_energy / the restrained path loop; formulas in
include/hierdiff_hip.h, "Restraint-guided sampling"), the yardstick of tests/test_restraint_cpu.py and tests/test_gpu_restraint.py.

Written from the formulas with plain Python loops over the rows: hand-derived gradients, nothing imported from the product but the
`Restraints` container that holds the tables.  The update starts from the fp32 data prediction x^0 = nv0 (1 / alpha) (z - sigma eps)
computed in torch fp32 with the kernel's three operations in the kernel's order; everything behind it is float64.  (The compiler
may contract z - sigma eps into one fused multiply-add on the device - the rounding intrinsics of k_chain_frame<1> are plain operators
in current ROCm headers - so the device's x^0 can differ from torch's by one unit in the last place; the magnitudes below count the
terms of x^0 itself, which covers it.)  Every function that returns a value also returns a MAGNITUDE: the same formula with every term replaced by its absolute
value and the mean by the mean of the absolute values - the scale tests/sampling_reference.py's element-wise bar is taken against.

`RestrainedNet` wraps a network of tests/edit_reference.py / tests/guidance_reference.py (anything with .net(z, t)) so that the
chain restatements of those modules and of tests/solver_reference.py run the restrained chain unchanged."""
import math

import numpy as np
import torch


def x0_f32(z, eps, alpha, sigma, nv0):
    """[B,N,3] float32: the kernel's operations in the kernel's order (divide, multiply, subtract, multiply, multiply by nv0)."""
    f = lambda v: torch.tensor(float(v), dtype=torch.float32)
    ra = f(1.0) / f(alpha)
    zx, ex = z[:, :, :3].to(torch.float32), eps[:, :, :3].to(torch.float32)
    return (ra * (zx - f(sigma) * ex)) * f(nv0)


def _row(t, b):
    return t[0 if t.shape[0] == 1 else b]


def energy_grad(rs, x, nm, xa=None):
    """x [B,N,3] (any float dtype; evaluated in float64), nm [B,N] bool-like.  Returns U [B,3] (obs, pair, anc), its magnitude (equal:
    every term is >= 0), g [B,N,3] = dU/dx and the magnitude of g.  The magnitude is the gradient's formula with every term replaced
    by its absolute value, differences expanded: a term k (d - r) / d (x_i - y) counts k (d + r) / d (|x_i| + |y|), with |x_i| the
    magnitude `xa` of the position itself (default |x|; the update passes nv0 (|z| + sigma |eps|) / alpha)."""
    x = np.asarray(x, dtype=np.float64)
    xa = np.abs(x) if xa is None else np.asarray(xa, dtype=np.float64)
    nm = np.asarray(nm).reshape(x.shape[0], x.shape[1]) != 0
    B, N = nm.shape
    U, g, ga = np.zeros((B, 3)), np.zeros((B, N, 3)), np.zeros((B, N, 3))

    def add(b, i, k, d, r, u, ua):
        g[b, i] += k * (d - r) / d * u
        ga[b, i] += k * (d + r) / d * ua

    for b in range(B):
        for (yx, yy, yz, r, k) in np.asarray(_row(rs.obs, b), dtype=np.float64):
            if not (r > 0 and k > 0):
                continue
            for i in range(N):
                if not nm[b, i]:
                    continue
                u = x[b, i] - np.array([yx, yy, yz])
                d = math.sqrt(float(u @ u))
                if d < r:
                    U[b, 0] += 0.5 * k * (r - d) ** 2
                    if d > 0:
                        add(b, i, k, d, r, u, xa[b, i] + np.abs([yx, yy, yz]))
        pi, pf = np.asarray(_row(rs.pair_idx, b)), np.asarray(_row(rs.pair_f, b), dtype=np.float64)
        for (i, j), (lo, hi, k) in zip(pi, pf):
            if i < 0 or j < 0 or i >= N or j >= N or i == j or not (nm[b, i] and nm[b, j]) or not k > 0:
                continue
            u = x[b, i] - x[b, j]
            d = math.sqrt(float(u @ u))
            v = d - hi if d > hi else (d - lo if d < lo else 0.0)
            U[b, 1] += 0.5 * k * v * v
            if v != 0.0 and d > 0:
                add(b, i, k, d, d - v, u, xa[b, i] + xa[b, j])
                add(b, j, k, d, d - v, -u, xa[b, i] + xa[b, j])
        ai, af = np.asarray(_row(rs.anc_idx, b)), np.asarray(_row(rs.anc_f, b), dtype=np.float64)
        for i, (ax, ay, az, r, k) in zip(ai, af):
            if i < 0 or i >= N or not nm[b, i] or not k > 0:
                continue
            u = x[b, i] - np.array([ax, ay, az])
            d = math.sqrt(float(u @ u))
            if d > r:
                U[b, 2] += 0.5 * k * (d - r) ** 2
                add(b, i, k, d, r, u, xa[b, i] + np.abs([ax, ay, az]))
    return U, U.copy(), g, ga


def project_step(g, ga, nm, sl, clip):
    """Delta [B,N,3] = s_b lambda g, clipped per node to length `clip` (inf: none), minus its mean over the valid nodes; and its
    magnitude.  sl [B] = s_b lambda."""
    nm = np.asarray(nm).reshape(g.shape[0], g.shape[1]) != 0
    sl = np.asarray(sl, dtype=np.float64).reshape(-1, 1, 1)
    d, da = sl * g, np.abs(sl) * ga
    if math.isfinite(clip):
        ln = np.sqrt((d * d).sum(-1, keepdims=True))
        f = np.where(ln > clip, clip / np.where(ln > 0, ln, 1.0), 1.0)
        d, da = d * f, da * f
    m = nm[:, :, None].astype(np.float64)
    cnt = np.maximum(m.sum(1, keepdims=True), 1.0)
    d, da = d * m, da * m
    return (d - d.sum(1, keepdims=True) / cnt) * m, (da + da.sum(1, keepdims=True) / cnt) * m


def restrain_ref(rs, z, eps, nm, scale, row4, nv0):
    """The update of one transition: (out [B,N,D] float64, magnitude [B,N,D]).  row4 = (alpha_t, sigma_t, lambda_k, clip_k) as the
    float32 values the kernel is given; scale: [1] or [B].  Molecules with s_b lambda_k == 0 keep eps exactly."""
    B, N, D = eps.shape
    al, sg, lam, clip = (float(np.float32(v)) for v in row4)
    s = np.asarray(torch.as_tensor(scale, dtype=torch.float32).reshape(-1).numpy(), dtype=np.float64)
    s = np.broadcast_to(s, (B,)) if s.size == 1 else s
    x0 = x0_f32(z, eps, al, sg, nv0).numpy()
    xa = (np.abs(z[:, :, :3].double().numpy()) + sg * np.abs(eps[:, :, :3].double().numpy())) * (nv0 / al)
    _, _, g, ga = energy_grad(rs, x0, nm, xa)
    d, da = project_step(g, ga, nm, s * lam, clip)
    out = eps.detach().double().numpy().copy()
    mag = np.abs(out)
    out[:, :, :3] += d
    mag[:, :, :3] += da
    return out, mag


class RestrainedNet:
    """eps^ of a restrained network call: `inner` has .net(z, t_idx) (a RefNet, a GuidedNet); `rows` maps the grid index t of a
    transition's departure level to its (alpha_t, sigma_t, lambda_k, clip_k).  A grid index without a row (the decode's t = 0) is the
    network's own.  The result is rounded once to the inner network's dtype, as the kernel writes fp32."""

    def __init__(self, inner, rs, scale, rows, nv0=1.0):
        self.inner, self.rs, self.scale, self.rows, self.nv0 = inner, rs, scale, dict(rows), float(nv0)
        self.dtype, self.nm = inner.dtype, inner.nm
        self.c = getattr(inner, "c", inner)          # the RefNet `ancestral_on_eps` / `decode_on_eps` take their masks from

    def net(self, z, t_idx):
        eps = self.inner.net(z, t_idx)
        if int(t_idx) not in self.rows:
            return eps
        out, _ = restrain_ref(self.rs, z, eps, self.nm, self.scale, self.rows[int(t_idx)], self.nv0)
        return torch.from_numpy(out).to(self.dtype)


def rows_from_grid(gg, path, schedule="score", clip=math.inf, nv0=1.0):
    """{t: (alpha_t, sigma_t, lambda_k, clip)} from the gamma grid in Python floats (math module): alpha / sigma are the fp32
    sqrt(sigmoid(-+gamma)) of the fp32 grid value, lambda the float64 expression rounded once."""
    out = {}
    for k, t in enumerate(path[:-1]):
        g32 = torch.as_tensor(gg, dtype=torch.float32).reshape(-1)[t]
        al32, sg32 = float(torch.sqrt(torch.sigmoid(-g32))), float(torch.sqrt(torch.sigmoid(g32)))
        g = float(gg[t])
        al, sg = math.sqrt(1.0 / (1.0 + math.exp(g))), math.sqrt(1.0 / (1.0 + math.exp(-g)))
        lam = nv0 * sg / al if schedule == "score" else (sg if schedule == "sigma" else float(schedule[k]))
        out[int(t)] = (al32, sg32, float(np.float32(lam)), float(clip))
    return out


# ----------------------------------------------------------------------------- the shared cases

def seven_node_case():
    """The fixed 7-node case with all three kinds of term: (Restraints, x [1,7,3] float64, nm [1,7])."""
    from hierdiff_amd.restraints import Restraints
    g = torch.Generator().manual_seed(11)
    x = torch.randn(1, 7, 3, generator=g, dtype=torch.float64) * 1.5
    x = x - x.mean(1, keepdim=True)
    y = (x[0, 3] + torch.tensor([0.4, -0.3, 0.2], dtype=torch.float64)).tolist()      # node 3 lies inside this obstacle
    rs = Restraints(obstacles=[y + [1.5, 3.0], [1.5, 1.0, -0.5, 1.2, 1.0], [0, 0, 0, 0, 1.0]],
                    pairs=[[0, 1, 0.5, 1.0, 2.0], [2, 5, 4.0, 5.0, 1.5], [3, 4, 0.0, 9.0, 1.0], [-1, -1, 0, 0, 0]],
                    anchors=[[6, 2.0, 2.0, 2.0, 0.5, 2.5], [1, 0.0, 0.0, 0.0, 0.1, 1.0], [-1, 0, 0, 0, 0, 0]])
    return rs, x, torch.ones(1, 7, dtype=torch.bool)


def random_tables(B, N, P, Q, A, seed, per_molecule):
    """Restraints with P / Q / A rows (padding rows, indices >= N and - through the mask - masked indices included), shared or per
    molecule, plus one obstacle centred exactly on a point the caller may place a node at (returned)."""
    from hierdiff_amd.restraints import Restraints
    rng = np.random.Generator(np.random.PCG64(seed))
    R = B if per_molecule else 1
    obs = np.zeros((R, P, 5))
    obs[:, :, :3] = rng.normal(0, 1.5, (R, P, 3))
    obs[:, :, 3] = rng.uniform(0.5, 2.5, (R, P))
    obs[:, :, 4] = rng.uniform(0.5, 3.0, (R, P))
    centre = None
    if P > 0:
        centre = obs[0, 0, :3].copy()
        obs[:, 0, :3] = centre
    if P > 2:
        obs[:, 2, 3] = 0.0                                        # padding
    prs = np.zeros((R, Q, 5))
    for r in range(R):
        for q in range(Q):
            i = int(rng.integers(0, N + 2))                       # may be >= N
            j = int(rng.integers(0, N + 2))
            j = j if j != i else (i + 1)
            lo = rng.uniform(0.0, 2.0)
            prs[r, q] = (i, j, lo, lo + rng.uniform(0.0, 1.0), rng.uniform(0.5, 2.0))
    if Q > 1:
        prs[:, 1] = (-1, -1, 0, 0, 0)
    anc = np.zeros((R, A, 6))
    for r in range(R):
        for a in range(A):
            anc[r, a] = (int(rng.integers(0, N + 1)),) + tuple(rng.normal(0, 2.0, 3)) + (rng.uniform(0.0, 0.5), rng.uniform(0.5, 2.0))
    sq = (lambda t: t) if per_molecule else (lambda t: t[0])
    return Restraints(sq(obs) if P else None, sq(prs) if Q else None, sq(anc) if A else None), centre
