"""Float64 restatement of diverse sampling (hd_diverse_eps / hd_diversity_energy / the diverse path loop; formulas in
include/hierdiff_hip.h, "Diverse sampling"), the yardstick of tests/test_diversity_cpu.py and tests/test_gpu_diversity.py.

Written from the formulas with plain Python loops over the pairs of a group; nothing is imported from the product.  The rotation comes
from numpy's SVD with the determinant fix - independent of the kernel's Jacobi iteration on Horn's quaternion matrix.  The update
starts from the fp32 data prediction of `restraint_reference.x0_f32`; everything behind it is float64.

CONDITIONING.  The gradient is exact without dR/dx, but R itself is as well determined as the two largest "signed" singular values
of S are apart from degeneracy: with S = U diag(s_1 >= s_2 >= s_3) V^T and d = det(U V^T), `cond` = (s_2 + d s_3) / s_1 (the measure
of tests/template_reference.py).  Every contributing pair of a compared case keeps cond >= COND_MIN: `kernel_cases` re-seeds until all
do, with a margin, and no case is left out.  The named degenerate cases (two common nodes, collinear nodes) are compared in d2 only.

MAGNITUDES follow tests/restraint_reference.py: every term replaced by its absolute value, every difference expanded - r_i counts
|x_p,i| + mean_A |x_p| + sum_j |R_cj| (|x_q,i,j| + mean_A |x_q,j|), with |x| the magnitude `xa` of the data prediction's own terms.

THE KERNEL'S x^0.  As in tests/template_reference.py the kernel cases use sigma_t = 0.5, so `x0_f32` is the kernel's x^0 bit for bit.

THE FP32 TWIN (`twin=True`): the same expressions in the number formats the kernel keeps - x^0 in fp32, sums in double, the written
element rounded once to fp32 - with the rotation from the largest eigenvector of Horn's 4x4 matrix (numpy eigh), a third route
next to the SVD and the kernel's Jacobi sweeps.

MUTANTS: `mutant=` names one deliberate mistake; tests/test_diversity_cpu.py asserts that each of them misses the GPU bar on the
inputs of the kernel test (`kernel_cases`)."""
import math

import numpy as np
import torch

from tests.restraint_reference import x0_f32

U = 2.0 ** -23
BOUND = 8.0
COND_MIN = 0.05
MUTANTS = ("sign", "no_n", "no_l2", "q_transposed", "no_det", "clip_element", "mean_all", "whole_batch")
ROW = (0.8, 0.5, 0.7)                   # alpha_t, sigma_t (exact products in fp32), lambda_k
NV0 = 1.7


def rotation_svd(S, mutant=None):
    """(R, cond) for S [3,3] = sum x' y'^T."""
    Um, s, Vt = np.linalg.svd(S)
    d = 1.0 if np.linalg.det(Um @ Vt) >= 0 else -1.0
    R = Um @ np.diag([1.0, 1.0, 1.0 if mutant == "no_det" else d]) @ Vt
    return R, float((s[1] + d * s[2]) / s[0]) if s[0] > 0 else 0.0


def rotation_horn(S):
    """R from the eigenvector of the largest eigenvalue of Horn's symmetric 4x4 matrix (numpy eigh)."""
    (xx, xy, xz), (yx, yy, yz), (zx, zy, zz) = S
    K = np.array([[xx + yy + zz, zy - yz, xz - zx, yx - xy], [zy - yz, xx - yy - zz, xy + yx, zx + xz],
                  [xz - zx, xy + yx, -xx + yy - zz, yz + zy], [yx - xy, zx + xz, yz + zy, -xx - yy + zz]])
    q0, q1, q2, q3 = np.linalg.eigh(K)[1][:, -1]
    return np.array([[q0 * q0 + q1 * q1 - q2 * q2 - q3 * q3, 2 * (q1 * q2 - q0 * q3), 2 * (q1 * q3 + q0 * q2)],
                     [2 * (q1 * q2 + q0 * q3), q0 * q0 - q1 * q1 + q2 * q2 - q3 * q3, 2 * (q2 * q3 - q0 * q1)],
                     [2 * (q1 * q3 - q0 * q2), 2 * (q2 * q3 + q0 * q1), q0 * q0 - q1 * q1 - q2 * q2 + q3 * q3]])


def pair_fit(xp, xq, mp, mq, xap=None, xaq=None, mutant=None, twin=False):
    """The fit of rows xp, xq [N,3] under the masks mp, mq [N]: None when the pair contributes nothing, else a dict with the common
    nodes `idx`, n, the residuals of both sides rp / rq [n,3] and their magnitudes, d2 and cond."""
    a = np.flatnonzero(mp & mq)
    n = len(a)
    if n <= 1 or not (np.isfinite(xp[a]).all() and np.isfinite(xq[a]).all()):
        return None
    xap = np.abs(xp) if xap is None else xap
    xaq = np.abs(xq) if xaq is None else xaq
    P_, Q_ = xp[a] - xp[a].mean(0), xq[a] - xq[a].mean(0)
    Pa, Qa = xap[a] + xap[a].mean(0), xaq[a] + xaq[a].mean(0)
    S = P_.T @ Q_
    R, cond = rotation_svd(S, mutant)
    if twin and mutant != "no_det":
        R = rotation_horn(S)
    rp = P_ - Q_ @ R.T                                 # (x_p - c_p) - R (x_q - c_q)
    Rq = R if mutant == "q_transposed" else R.T
    rq = Q_ - P_ @ Rq.T                                # (x_q - c_q) - R^T (x_p - c_p)
    return dict(idx=a, n=n, R=R, cond=cond, rp=rp, rq=rq, rpa=Pa + Qa @ np.abs(R).T, rqa=Qa + Pa @ np.abs(Rq).T,
                d2=float((rp * rp).sum() / n))


def phi_grad(x, nm, P, kappa, length, xa=None, mutant=None, twin=False):
    """x [B,N,3] (evaluated in float64), nm [B,N] bool-like, groups of P rows.  Returns Phi [G], rmsd [G,P,P] (NaN: the pair contributes
    nothing), g [B,N,3] = dPhi/dx, its magnitude, and the conditioning measures of the contributing pairs."""
    x = np.asarray(x, dtype=np.float64)
    xa = np.abs(x) if xa is None else np.asarray(xa, dtype=np.float64)
    nm = np.asarray(nm).reshape(x.shape[0], x.shape[1]) != 0
    B, N = nm.shape
    G = B // P
    phi, rmsd = np.zeros(G), np.full((G, P, P), np.nan)
    g, ga, conds = np.zeros((B, N, 3)), np.zeros((B, N, 3)), []
    l2 = 1.0 if mutant == "no_l2" else length * length
    sign = 1.0 if mutant == "sign" else -1.0
    for b in range(B):
        grp = b // P
        rmsd[grp, b % P, b % P] = 0.0
        partners = range(B) if mutant == "whole_batch" else range(grp * P, grp * P + P)
        for o in partners:                                 # ascending
            if o == b:
                continue
            p, q = min(b, o), max(b, o)
            f = pair_fit(x[p], x[q], nm[p], nm[q], xa[p], xa[q], mutant, twin)
            if f is None:
                continue
            e = math.exp(-f["d2"] / (2.0 * length * length))
            w = kappa * e / (l2 * (1.0 if mutant == "no_n" else f["n"]))
            r, ra = (f["rp"], f["rpa"]) if b == p else (f["rq"], f["rqa"])
            g[b, f["idx"]] += sign * w * r
            ga[b, f["idx"]] += w * ra
            if b == p and o // P == grp:
                phi[grp] += kappa * e
                rmsd[grp, p % P, q % P] = rmsd[grp, q % P, p % P] = math.sqrt(f["d2"])
                conds.append(f["cond"])
    return phi, rmsd, g, ga, conds


def project_step(g, ga, nm, sl, clip, mutant=None):
    """Delta [B,N,3] = s lambda g, clipped per node to length `clip` (inf: none), minus its mean over the valid nodes; and its magnitude.
    sl [B] = s_g lambda of every row."""
    nm = np.asarray(nm).reshape(g.shape[0], g.shape[1]) != 0
    sl = np.asarray(sl, dtype=np.float64).reshape(-1, 1, 1)
    d, da = sl * g, np.abs(sl) * ga
    if math.isfinite(clip):
        if mutant == "clip_element":
            f = np.where(np.abs(d) > clip, clip / np.where(d != 0, np.abs(d), 1.0), 1.0)
        else:
            ln = np.sqrt((d * d).sum(-1, keepdims=True))
            f = np.where(ln > clip, clip / np.where(ln > 0, ln, 1.0), 1.0)
        d, da = d * f, da * f
    m = nm[:, :, None].astype(np.float64)
    cnt = np.full((g.shape[0], 1, 1), float(g.shape[1])) if mutant == "mean_all" else np.maximum(m.sum(1, keepdims=True), 1.0)
    d, da = d * m, da * m
    return (d - d.sum(1, keepdims=True) / cnt) * m, (da + da.sum(1, keepdims=True) / cnt) * m


def data_prediction(c):
    return x0_f32(c.z, c.eps, c.row[0], c.row[1], c.nv0).double().numpy()


def diverse_ref(z, eps, nm, P, kappa, length, scale, row4, nv0, mutant=None, twin=False):
    """The update of one transition: (out [B,N,D] float64, magnitude [B,N,D]).  row4 = (alpha_t, sigma_t, lambda_k, clip_k) as the
    float32 values the kernel is given; scale: [1] or [G].  Groups with s_g lambda_k == 0 keep eps exactly.  `twin`: the fp32 twin."""
    B, N, D = eps.shape
    al, sg, lam, clip = (float(np.float32(v)) for v in row4)
    s = np.asarray(torch.as_tensor(scale, dtype=torch.float32).reshape(-1).numpy(), dtype=np.float64)
    s = np.broadcast_to(s, (B // P,)) if s.size == 1 else s
    x0 = x0_f32(z, eps, al, sg, nv0).double().numpy()
    xa = (np.abs(z[:, :, :3].double().numpy()) + sg * np.abs(eps[:, :, :3].double().numpy())) * (nv0 / al)
    _, _, g, ga, _ = phi_grad(x0, nm, P, kappa, length, xa, mutant, twin)
    d, da = project_step(g, ga, nm, np.repeat(s, P) * lam, clip, mutant)
    out = eps.detach().double().numpy().copy()
    mag = np.abs(out)
    out[:, :, :3] += d
    mag[:, :, :3] += da
    if twin:
        out = out.astype(np.float32).astype(np.float64)
    return out, mag


class DiverseNet:
    """eps^ of a diverse network call: `inner` has .net(z, t_idx); `rows` maps the grid index t of a transition's departure level to
    its (alpha_t, sigma_t, lambda_k, clip_k).  A grid index without a row (the decode's t = 0) is the network's own.  The result is
    rounded once to the inner network's dtype, as the kernel writes fp32.  Counts the calls in which the term changed eps^."""

    def __init__(self, inner, P, kappa, length, scale, rows, nv0=1.0):
        self.inner, self.P, self.kappa, self.length, self.scale, self.rows, self.nv0 = inner, P, kappa, length, scale, dict(rows), float(nv0)
        self.dtype, self.nm = inner.dtype, inner.nm
        self.c = getattr(inner, "c", inner)
        self.calls = self.active = 0

    def net(self, z, t_idx):
        eps = self.inner.net(z, t_idx)
        if int(t_idx) not in self.rows:
            return eps
        out, _ = diverse_ref(z, eps, self.nm, self.P, self.kappa, self.length, self.scale, self.rows[int(t_idx)], self.nv0)
        out = torch.from_numpy(out).to(self.dtype)
        self.calls += 1
        self.active += int(not torch.equal(out, eps.to(self.dtype)))
        return out


# ----------------------------------------------------------------------------- the shared cases

class Case:
    pass


def _rotation(rng):
    Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return Q if np.linalg.det(Q) > 0 else -Q


def _group_rows(rng, P, N, spread=0.45):
    """P rows that are rotated, shifted and perturbed copies of one arrangement of N points - variants of a lead."""
    base = rng.normal(0.0, 1.5, (N, 3))
    return np.stack([(base + rng.normal(0.0, spread, (N, 3))) @ _rotation(rng).T + rng.normal(0.0, 0.3, 3) for _ in range(P)])


def _masks(kind, G, P, N):
    nm = np.ones((G * P, N), dtype=bool)
    if kind == "partly masked":                            # equal masks inside a group; group 1 keeps about half, group 2 two nodes more
        nm[P:2 * P, (N + 1) // 2:] = False
        nm[2 * P:, max(3, N - 2):] = False
    elif kind == "unequal masks":                          # rows of group 0 lose different nodes; the last row of group 1 is masked out
        for p in range(P):
            nm[p, (p * 2) % N] = False
        nm[2 * P - 1] = False
    elif kind == "one common node, none":
        # group 0: rows 0 and 1 share exactly node 0 (at least three nodes each, so their pairs with the full rows stay determined);
        # group 1: row 1 shares no node with any other row of its group
        h = (N - 1) // 2
        nm[0, h + 1:] = False
        nm[1, 1:h + 1] = False
        nm[P:2 * P, : N // 2] = False
        nm[P + 1] = ~nm[P]
    return nm


def make_case(G, P, N, D, kind="full", clip=math.inf, scale=None, seed=0, kappa=1.3, length=1.1):
    """One kernel case: z, eps [B,N,D] float32 whose data prediction under ROW / NV0 holds the rows of `_group_rows`."""
    rng = np.random.Generator(np.random.PCG64(seed))
    c = Case()
    c.G, c.P, c.N, c.D, c.B = G, P, N, D, G * P
    c.kappa, c.length, c.nv0 = kappa, length, NV0
    c.row = ROW + (clip,)
    c.nm = torch.from_numpy(_masks(kind, G, P, N))
    x = np.concatenate([_group_rows(rng, P, N) for _ in range(G)])
    if kind == "identical rows":
        x[1] = x[0]
    elif kind == "mirror image":
        x[1] = x[0] * np.array([1.0, 1.0, -1.0])
    elif kind == "two common nodes":
        c.nm[:P, 2:] = False
    elif kind == "collinear":
        t = np.linspace(-2.0, 2.0, N)[:, None]
        for p in range(P):
            x[p] = t * _rotation(rng)[0] * (1.0 + 0.1 * p) + rng.normal(0.0, 0.3, 3)
    # eps, then the z that puts x^0 = nv0 (z - sigma eps) / alpha on x (up to fp32 rounding)
    eps = rng.normal(0.0, 1.0, (c.B, N, D)).astype(np.float32)
    z = rng.normal(0.0, 1.0, (c.B, N, D)).astype(np.float32)
    z[:, :, :3] = (x * (ROW[0] / NV0) + ROW[1] * eps[:, :, :3].astype(np.float64)).astype(np.float32)
    if kind == "identical rows":
        z[1, :, :3], eps[1, :, :3] = z[0, :, :3], eps[0, :, :3]
    if kind == "nan coordinate":
        z[1, 0, 0] = np.nan
    c.z, c.eps = torch.from_numpy(z), torch.from_numpy(eps)
    c.scale = torch.ones(1) if scale is None else torch.as_tensor(scale, dtype=torch.float32)
    c.kind, c.degenerate = kind, kind in DEGENERATE
    c.name = f"G={G} P={P} N={N} D={D} {kind} clip={clip} scale_rows={c.scale.numel()}"
    return c


DEGENERATE = ("two common nodes", "collinear")
KINDS = ("full", "partly masked", "unequal masks", "one common node, none", "identical rows", "mirror image", "nan coordinate")
MARGIN = 1.5


def worst_cond(c):
    """The smallest conditioning measure over the pairs that contribute (inf: none does)."""
    return min(phi_grad(data_prediction(c), c.nm.numpy(), c.P, c.kappa, c.length)[4] + [math.inf])


def conditioned_case(*args, **kw):
    """`make_case`, re-seeded until every contributing pair clears MARGIN * COND_MIN (degenerate kinds: as drawn).  Returns the case
    and the number of seeds tried."""
    kind = kw.get("kind", "full")
    seed = kw.pop("seed", 0)
    for attempt in range(400):
        c = make_case(*args, seed=1000 * attempt + seed, **kw)
        if kind in DEGENERATE or worst_cond(c) >= MARGIN * COND_MIN:
            c.attempts = attempt + 1
            return c
    raise AssertionError(f"no seed gives well-conditioned pairs: {args} {kw}")


def kernel_cases(N, D):
    """The cases of the kernel parity test at one (N, D): G = 3; P in {2, 4, 8}; scale_rows in {1, G}; the clip finite and infinite;
    every kind of group; a group with scale 0; the degenerate kinds."""
    G = 3
    n = 0
    for P in (2, 4, 8):
        for kind in KINDS:
            if kind == "one common node, none" and P < 2:
                continue
            n += 1
            per = (n % 2 == 0)
            clip = 0.05 if n % 3 == 0 else math.inf
            scale = [1.0, 0.6, 0.8] if per else None
            yield conditioned_case(G, P, N, D, kind=kind, clip=clip, scale=scale, seed=n)
        yield conditioned_case(G, P, N, D, kind="full", clip=0.05, scale=[1.0, 0.0, 0.7], seed=50 + P)     # a group with scale 0
    for kind in DEGENERATE:
        yield conditioned_case(G, 4, N, D, kind=kind, seed=70)


def big_case():
    """P = 32 (496 pairs per group, two rounds of the pair loop) at N = 5."""
    return conditioned_case(3, 32, 5, 4, kind="full", clip=0.05, scale=[1.0, 0.6, 0.8], seed=90)
