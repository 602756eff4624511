"""Float64 restatement of the feature restraints (hd_restraint_features / hd_restrain_feat / hd_restraint_feature_energy and the
feature term of the restrained path loop; formulas in include/hierdiff_hip.h, "Feature restraints"), the yardstick of
tests/test_feature_cpu.py and tests/test_gpu_feature.py.

Written from the formulas with plain loops over molecules, nodes, channels and rows; nothing imported from the product but the
`Features` / `FeatureSum` / `Restraints` containers that hold the rows.  For a valid node i and channel c, everything in float64:

    v_ic = ((z - sigma eps) / alpha) nv1 + nb1
    bands   active when k_ic > 0 and v_ic finite:  U += 1/2 k (max(0, v - hi)^2 + max(0, lo - v)^2),  g_ic += k (max(0, v - hi) - max(0, lo - v))
    sums    s_r = sum_i sum_c coef_rc v_ic,  m_r = s_r or s_r / n;  active when k_r > 0, n > 0 and no v it reads (coef != 0) is non-finite:
            U += 1/2 k_r (max(0, m - hi)^2 + max(0, lo - m)^2),  g_ic += k_r (max(0, m - hi) - max(0, lo - m)) coef_rc (1 or 1 / n)
    update  eps_h[i, c] += clip_i(s_b lambda ratio g_ic), the clip on the Euclidean norm over the node's F steps; no mean is removed

`restrain_feat_ref` is that, v included, in float64.  `restrain_feat_twin` is the FP32 TWIN: v in torch fp32 with the kernel's five
operations in the kernel's order (divide, multiply, subtract, multiply, multiply by nv1, add nb1), the rest in double, the result
rounded to fp32 once - what a correct kernel computes up to the order of its sums.

MAGNITUDES follow tests/restraint_reference.py: every term replaced by its absolute value, every difference expanded.  |v| counts
(|z| + sigma |eps|) |nv1| / alpha + |nb1|; a band term k (v - bound) counts k (|v| + |bound|) (an infinite bound never enters: its
branch is not taken); m_r counts sum |coef| |v| (/ n); a clipped step keeps its factor.

MUTANTS: `mutant=` names one deliberate mistake; tests/test_feature_cpu.py asserts that each of them misses the GPU bars on the
inputs of the kernel test (`kernel_cases`)."""
import math

import numpy as np
import torch

MUTANTS = ("no_nb1", "nv1_after_bias", "mean_without_n", "clip_per_element", "lower_sign", "ratio_ignored", "masked_in_n")


def v_f32(z, eps, alpha, sigma, nv1, nb1):
    """[B,N,F] float32: the kernel's operations in the kernel's order."""
    f = lambda v: torch.tensor(float(v), dtype=torch.float32)
    ra = f(1.0) / f(alpha)
    zh, eh = z[:, :, 3:].to(torch.float32), eps[:, :, 3:].to(torch.float32)
    return ((ra * (zh - f(sigma) * eh)) * f(nv1)) + f(nb1)


def v_f64(z, eps, alpha, sigma, nv1, nb1, mutant=None):
    zh, eh = z[:, :, 3:].double().numpy(), eps[:, :, 3:].double().numpy()
    t = (zh - sigma * eh) / alpha
    with np.errstate(all="ignore"):
        if mutant == "no_nb1":
            return t * nv1
        if mutant == "nv1_after_bias":
            return (t + nb1) * nv1
        return t * nv1 + nb1


def v_mag(z, eps, alpha, sigma, nv1, nb1):
    with np.errstate(all="ignore"):
        return (np.abs(z[:, :, 3:].double().numpy()) + sigma * np.abs(eps[:, :, 3:].double().numpy())) * (abs(nv1) / alpha) + abs(nb1)


def _rows(t, b):
    return np.asarray(t[0 if t.shape[0] == 1 else b].numpy(), dtype=np.float64)


def _excess(v, lo, hi, mutant=None):
    """(d, magnitude of d) with dU/dv = k d and U = 1/2 k d^2."""
    if v > hi:
        return v - hi, abs(hi)
    if v < lo:
        return (lo - v if mutant == "lower_sign" else v - lo), abs(lo)
    return 0.0, 0.0


def feature_energy_grad(ft, v, nm, va=None, mutant=None):
    """v [B,N,F] features in data units, nm [B,N].  Returns U [B,2] = (U_band, U_sum), g [B,N,F] = dU_feat/dv, the magnitude of g, m
    [B,S] (0 for a row that is inactive or contributes nothing) and the magnitude of m."""
    v = np.asarray(v, dtype=np.float64)
    B, N, F = v.shape
    va = np.abs(v) if va is None else np.asarray(va, dtype=np.float64)
    nm = np.asarray(nm).reshape(B, N) != 0
    S = len(ft.sums)
    U, g, ga = np.zeros((B, 2)), np.zeros((B, N, F)), np.zeros((B, N, F))
    m_out, mm_out = np.zeros((B, S)), np.zeros((B, S))
    for b in range(B):
        valid = [i for i in range(N) if nm[b, i]]
        n = float(N if mutant == "masked_in_n" else len(valid))
        if ft.lo is not None:
            lo, hi, k = _rows(ft.lo, b), _rows(ft.hi, b), _rows(ft.k, b)
            for i in valid:
                if i >= lo.shape[0]:
                    continue
                for c in range(F):
                    if not (k[i, c] > 0) or not math.isfinite(v[b, i, c]):
                        continue
                    d, bm = _excess(v[b, i, c], lo[i, c], hi[i, c], mutant)
                    U[b, 0] += 0.5 * k[i, c] * d * d
                    if d != 0.0:
                        g[b, i, c] += k[i, c] * d
                        ga[b, i, c] += k[i, c] * (va[b, i, c] + bm)
        for r, row in enumerate(ft.sums):
            coef = np.asarray(row.coef.numpy(), dtype=np.float64)
            rlo, rhi = float(_rows(row.lo, b)), float(_rows(row.hi, b))
            k = float(row.k)
            if not k > 0 or not valid:
                continue
            s = sm = 0.0
            bad = False
            for i in valid:
                for c in range(F):
                    if coef[c] == 0.0:
                        continue
                    if not math.isfinite(v[b, i, c]):
                        bad = True
                        continue
                    s += coef[c] * v[b, i, c]
                    sm += abs(coef[c]) * va[b, i, c]
            if bad:
                continue
            mean = row.reduce == "mean"
            w = 1.0 / n if mean else 1.0
            m, mm = (s, sm) if (not mean or mutant == "mean_without_n") else (s / n, sm / n)
            if mutant == "mean_without_n":
                w = 1.0
            m_out[b, r], mm_out[b, r] = m, mm
            d, bm = _excess(m, rlo, rhi, mutant)
            U[b, 1] += 0.5 * k * d * d
            if d != 0.0:
                for i in valid:
                    g[b, i] += k * d * w * coef
                    ga[b, i] += k * (mm + bm) * w * np.abs(coef)
    return U, g, ga, m_out, mm_out


def clip_step(g, ga, nm, sl, clip, mutant=None):
    """Delta [B,N,F] = s_b lambda^h g on valid nodes, clipped per node to the Euclidean length `clip` (inf: none); and its magnitude."""
    B, N, F = g.shape
    nm = np.asarray(nm).reshape(B, N) != 0
    sl = np.asarray(sl, dtype=np.float64).reshape(-1, 1, 1)
    d, da = sl * g, np.abs(sl) * ga
    if math.isfinite(clip):
        ln = np.abs(d) if mutant == "clip_per_element" else np.sqrt((d * d).sum(-1, keepdims=True))
        f = np.where(ln > clip, clip / np.where(ln > 0, ln, 1.0), 1.0)
        d, da = d * f, da * f
    m = nm[:, :, None].astype(np.float64)
    return d * m, da * m


def _scales(scale, B):
    s = np.asarray(torch.as_tensor(scale, dtype=torch.float32).reshape(-1).numpy(), dtype=np.float64)
    return np.broadcast_to(s, (B,)) if s.size == 1 else s


def restrain_feat_ref(ft, z, eps, nm, scale, row4, nv1, nb1, ratio, mutant=None, v=None):
    """The feature update of one transition in float64: (out [B,N,D] float64, magnitude [B,N,D]).  row4 = (alpha_t, sigma_t,
    lambda_k, clip_k) as the float32 values the kernel is given; scale [1] or [B]; nv1, nb1, ratio as fp32 values.  Molecules with
    s_b lambda^h == 0 keep eps exactly.  `v`: evaluate on these features instead (the twin)."""
    B, N, D = eps.shape
    al, sg, lam, clip = (float(np.float32(x)) for x in row4)
    nv1, nb1, ratio = (float(np.float32(x)) for x in (nv1, nb1, ratio))
    s = _scales(scale, B)
    v = v_f64(z, eps, al, sg, nv1, nb1, mutant) if v is None else np.asarray(v, dtype=np.float64)
    va = v_mag(z, eps, al, sg, nv1, nb1)
    _, g, ga, _, _ = feature_energy_grad(ft, v, nm, va, mutant)
    lamh = lam if mutant == "ratio_ignored" else lam * ratio
    d, da = clip_step(g, ga, nm, s * lamh, clip, mutant)
    out = eps.detach().double().numpy().copy()
    mag = np.abs(out)
    out[:, :, 3:] += d
    mag[:, :, 3:] += da
    return out, mag


def restrain_feat_twin(ft, z, eps, nm, scale, row4, nv1, nb1, ratio):
    """The fp32 twin: v in fp32 with the kernel's operations, the rest in double, rounded to fp32 once ([B,N,D] float32 tensor)."""
    al, sg = float(np.float32(row4[0])), float(np.float32(row4[1]))
    v = v_f32(z, eps, al, sg, nv1, nb1).numpy()
    out, _ = restrain_feat_ref(ft, z, eps, nm, scale, row4, nv1, nb1, ratio, v=v)
    res = torch.from_numpy(out).to(torch.float32)
    same = torch.from_numpy(out) == eps.double()              # an unmoved entry keeps its bits (a NaN of eps never equals: copied below)
    return torch.where(same | torch.isnan(eps), eps.to(torch.float32), res)


class FeatNet:
    """eps^ of a network call behind the restraint update with features: `inner` has .net(z, t_idx) and does the position update, if
    any (a RefNet, a GuidedNet, a `restraint_reference.RestrainedNet`, ...); `rows` maps the grid index t of a transition's departure
    level to its (alpha_t, sigma_t, lambda_k, clip_k).  Counts the calls in which the feature term moved eps^ (`active`)."""

    def __init__(self, inner, ft, scale, rows, nv1, nb1, ratio, nm=None):
        self.inner, self.ft, self.scale, self.rows = inner, ft, scale, dict(rows)
        self.nv1, self.nb1, self.ratio = float(nv1), float(nb1), float(ratio)
        self.dtype, self.nm = inner.dtype, inner.nm if nm is None else nm
        self.c = getattr(inner, "c", inner)
        self.active = self.calls = 0

    def net(self, z, t_idx):
        eps = self.inner.net(z, t_idx)
        if int(t_idx) not in self.rows:
            return eps
        out, _ = restrain_feat_ref(self.ft, z, eps, self.nm, self.scale, self.rows[int(t_idx)], self.nv1, self.nb1, self.ratio)
        self.calls += 1
        self.active += int(np.abs(out - eps.double().numpy()).max() > 0)
        return torch.from_numpy(out).to(self.dtype)


# ----------------------------------------------------------------------------- the shared cases

ROW = (0.8, 0.5, 0.75)                  # alpha_t, sigma_t (a power of two: sigma eps is exact in fp32), lambda_k of the kernel cases
NV0, NV1, NB1, RATIO = 1.7, 1.7, 0.3, 0.625
B = 5                                   # ordinary, s_b = 0, one valid node, no valid node, a NaN in one valid feature element
SCALE = (1.0, 0.0, 2.0, 1.5, 0.5)
NAN_AT = (4, 1, 0)                      # molecule, node, channel of the NaN (in z)


class _Case:
    pass


def masks_for(N):
    nm = torch.zeros(B, N, dtype=torch.bool)
    for b, n in enumerate((N, (N + 1) // 2, 1, 0, max(2, N - 1))):
        nm[b, :n] = True
    return nm


def base_case(N, F):
    c = _Case()
    c.B, c.N, c.F, c.D = B, N, F, F + 3
    c.nm = masks_for(N)
    g = torch.Generator().manual_seed(N * 100 + F)
    c.z, c.eps = torch.randn(B, N, c.D, generator=g), torch.randn(B, N, c.D, generator=g)
    c.z[NAN_AT[0], NAN_AT[1], 3 + NAN_AT[2]] = float("nan")
    c.scale = torch.tensor(SCALE)
    c.nv0, c.nv1, c.nb1, c.ratio = NV0, NV1, NB1, RATIO
    return c


def make_features(c, W, S, per, seed, row):
    """Bands on the first W nodes around the case's own data prediction, so that about half of the active elements lie outside their
    band and a good part inside; element (0, 0) of molecule 0 sits exactly on its upper bound and, with F > 1, (0, F - 1) on its lower one (the fp32
    v); some elements carry k = 0, one-sided bands and a harmonic target (lo = hi).  S sum rows, both reduce modes alternating, each
    row's window placed between the molecules' values of m_r so that it is violated in some molecules and satisfied in others."""
    from hierdiff_amd.restraints import Features, FeatureSum
    rng = np.random.Generator(np.random.PCG64(seed))
    N, F = c.N, c.F
    v = v_f32(c.z, c.eps, row[0], row[1], c.nv1, c.nb1).numpy().astype(np.float64)
    R = B if per else 1
    lo = hi = k = None
    if W:
        centre = np.where(np.isfinite(v[:R, :W]), v[:R, :W], 0.0) if per else np.where(np.isfinite(v[0, :W]), v[0, :W], 0.0)[None]
        half = rng.uniform(0.2, 1.0, (R, W, F))
        outside = rng.uniform(0.0, 1.0, (R, W, F)) < 0.65    # of the molecule the band was built on; the others fall where they fall
        off = np.where(outside, half + rng.uniform(0.1, 1.0, (R, W, F)), 0.9 * half * rng.uniform(0.0, 1.0, (R, W, F)))
        off = off * rng.choice([-1.0, 1.0], (R, W, F))
        lo, hi = centre + off - half, centre + off + half
        k = rng.uniform(0.5, 2.0, (R, W, F))
        kind = rng.integers(0, 8, (R, W, F))
        lo[kind == 0], hi[kind == 1] = -np.inf, np.inf        # one-sided
        hi[kind == 2] = lo[kind == 2]                         # a harmonic target
        k[kind == 3] = 0.0                                    # inactive
        hi[0, 0, 0] = v[0, 0, 0]                              # molecule 0 (valid, finite) exactly on the upper bound
        lo[0, 0, 0] = hi[0, 0, 0] - 1.0
        if F > 1:                                             # ... and on the lower one
            lo[0, 0, F - 1] = v[0, 0, F - 1]
            hi[0, 0, F - 1] = lo[0, 0, F - 1] + 1.0
        k[0, 0, 0] = k[0, 0, F - 1] = 1.25
        lo, hi = np.where(np.isnan(lo), 0.0, lo), np.where(np.isnan(hi), 1.0, hi)
        lo, hi = np.minimum(lo, hi), np.maximum(lo, hi)
    sums = []
    nmn = c.nm.numpy()
    for r in range(S):
        coef = rng.normal(0.0, 1.0, F)
        if F > 2 and r % 3 == 1:
            coef[rng.integers(0, F)] = 0.0                    # a channel the row does not read
        if r == S - 1 and F > 1:
            coef[NAN_AT[2]] = 0.0                             # this row does not read the NaN: it stays live in that molecule
        coef = np.asarray(coef, dtype=np.float32).astype(np.float64)
        reduce = "mean" if r % 2 else "sum"
        ms = []
        for b in range(B):
            n = int(nmn[b].sum())
            if n == 0 or SCALE[b] == 0.0:
                continue
            vb = v[b][nmn[b]]
            if not np.isfinite(vb[:, coef != 0]).all():
                continue
            s = float(np.where(coef != 0, vb * coef, 0.0).sum())
            ms.append(s / n if reduce == "mean" else s)
        ms = sorted(ms)
        a, bb = ms[0], ms[-1]                                 # at least two live molecules: the ordinary one and the single node
        mid, w = 0.5 * (a + bb), bb - a
        if (r // 2) % 2:                                      # the largest value inside, the smallest below the window
            wlo, whi = mid, bb + 0.5 * w
            if r % 4 == 3:
                whi = None                                    # one-sided
        else:                                                 # the smallest value inside, the largest above the window
            wlo, whi = a - 0.5 * w, mid
            if r % 4 == 0 and r > 0:
                wlo = None
        if per:
            wlo = None if wlo is None else np.full(B, wlo)
            whi = None if whi is None else np.full(B, whi)
        sums.append(FeatureSum(coef, wlo, whi, k=float(rng.uniform(0.3, 1.5)), reduce=reduce))
    if W:
        return Features(lo if per else lo[0], hi if per else hi[0], k if per else k[0], sums)
    return Features(sums=sums)


def conditions_hold(c):
    """At least a quarter of the active band elements outside their band, a tenth inside, one exactly on a bound; every sum row
    violated in at least one molecule and satisfied in at least one."""
    out_, in_, on, rows = input_conditions(c)
    return (c.ft.lo is None or (out_ >= 0.25 and in_ >= 0.1 and on >= 1)) and all(v > 0 and s > 0 for v, s in rows)


def _conditioned(c, W, S, per, seed):
    """c.ft: the first of the seeds seed, seed + 1000, ... whose features meet `conditions_hold` (a handful of elements at the small
    shapes: a single draw can miss a fraction)."""
    for attempt in range(100):
        c.ft = make_features(c, W, S, per, seed + 1000 * attempt, c.row)
        if conditions_hold(c):
            return
    raise AssertionError("no seed gives features that meet the input conditions")


def kernel_cases(N, F):
    """The inputs of the kernel tests at one shape: cases with .rs (a Restraints holding only features), .ft, .z, .eps, .nm, .scale,
    .row (4 floats), .nv1, .nb1, .ratio, .name.  W in {N - 2 (at least 1), N} x S in {0, 1, 8} x shared / per-molecule rows,
    alternating clip inf / finite so that every pair of settings occurs."""
    from hierdiff_amd.restraints import Restraints
    base = base_case(N, F)
    n = 0
    for W in (max(1, N - 2), N):
        for S in (0, 1, 8):
            for per in (False, True):
                c = _Case()
                c.__dict__.update(base.__dict__)
                clip = 0.4 if (n // 2 + n) % 2 else math.inf
                n += 1
                c.row = ROW + (clip,)
                _conditioned(c, W, S, per, 100 * N + 10 * F + n)
                c.rs = Restraints(features=c.ft)
                c.name = f"W={W} S={S} {'rows' if per else 'shared'} clip={clip}"
                yield c
    c = _Case()                                               # sums alone
    c.__dict__.update(base.__dict__)
    c.row = ROW + (0.4,)
    _conditioned(c, 0, 8, False, 7 * N + F)
    c.rs = Restraints(features=c.ft)
    c.name = "W=0 S=8 shared clip=0.4"
    yield c


def input_conditions(c):
    """What tests/test_feature_cpu.py asserts of every kernel case: (fraction of the active band elements outside their band, fraction
    inside, elements exactly on a bound, per sum row whether it is violated in some molecule and satisfied in some)."""
    v = v_f32(c.z, c.eps, c.row[0], c.row[1], c.nv1, c.nb1).numpy().astype(np.float64)
    nm = c.nm.numpy()
    out_ = in_ = on = 0
    ft = c.ft
    if ft.lo is not None:
        for b in range(B):
            lo, hi, k = _rows(ft.lo, b), _rows(ft.hi, b), _rows(ft.k, b)
            for i in range(min(c.N, lo.shape[0])):
                for ch in range(c.F):
                    if not nm[b, i] or not k[i, ch] > 0 or not math.isfinite(v[b, i, ch]):
                        continue
                    x = v[b, i, ch]
                    if x == lo[i, ch] or x == hi[i, ch]:
                        on += 1
                    if x > hi[i, ch] or x < lo[i, ch]:
                        out_ += 1
                    else:
                        in_ += 1
    rows = []
    _, _, _, m, _ = feature_energy_grad(ft, v, nm)
    for r, row in enumerate(ft.sums):
        viol = sat = 0
        for b in range(B):
            if not nm[b].any() or not np.isfinite(v[b][nm[b]][:, row.coef.numpy() != 0]).all():
                continue
            lo, hi = float(_rows(row.lo, b)), float(_rows(row.hi, b))
            if m[b, r] > hi or m[b, r] < lo:
                viol += 1
            else:
                sat += 1
        rows.append((viol, sat))
    tot = max(1, out_ + in_)
    return out_ / tot, in_ / tot, on, rows


# ----------------------------------------------------------------------------- the chains (T = 8, K = 4, B = 4) over the oracle
# The models of tests/test_gpu_restraint.py with other normalisation constants for h, so that nv1, nb1 and the ratio nv1 / nv0 of the
# "score" schedule take part: the network and the updates work in normalised units and do not see them.

CHAIN_T, CHAIN_K = 8, 4
CHAIN_SHAPES = {"fp32": (32, 2), "fp16x3": (128, 1)}
CHAIN_MOLS = (7, 4, 1, 6)
CHAIN_NORM = ([1.0, 1.7, 1.0], [None, 0.3, 0.0])             # norm_values, norm_biases
CHAIN_SCALE = (0.05, 0.02, 0.05, 0.08)
CHAIN_CLIP = 0.3
CHAIN_KINDS = ("features", "features+obstacles guided", "sde2m", "x0", "inpaint R=1", "inpaint R=2", "steered")
STEER_P, STEER_RHO, STEER_BETA, STEER_BASE, STEER_SEED = 4, 0.9, 1e-6, 24, 2022   # (U_feat ~ 1e6 at the noisy end: 1 / alpha_T is large)
INPAINT_BASE = 9
KNOWN_CENTRE = (12.0, -7.0, 30.0)


def chain_features(W=5, S=2, shift=0.0, rows=None, k=1.5):
    """Targets with a tolerance on the first W nodes (channel 0 of every node a harmonic one: active whatever the chain does), a
    ceiling on the molecule's sum of channel 2 and a window on the mean of channel 0."""
    from hierdiff_amd.restraints import Features, FeatureSum
    g = np.random.Generator(np.random.PCG64(17))
    val = g.normal(0.3, 1.5, (W, 8)) + shift
    tol = np.broadcast_to(np.array([0.0, 0.25, 0.5, 0.0, 0.25, 1.0, 0.0, 0.5]), (W, 8))
    kk = np.full((W, 8), k)
    kk[:, 7] = 0.0
    rep = (lambda a: a) if rows is None else (lambda a: np.broadcast_to(a, (rows,) + np.shape(a)).copy())
    sums = [FeatureSum([0, 0, 1, 0, 0, 0, 0, 0], hi=-3.0 + shift, k=0.5), FeatureSum([1, 0, 0, 0, 0, 0, 0, 0.5], lo=2.0, hi=2.5, k=2.0, reduce="mean"),
            FeatureSum([0, 1, 0, -1, 0, 0, 0, 0], lo=4.0, k=0.25)][:S]
    return Features.target(rep(val), rep(kk), rep(tol), sums)


def chain_obstacles():
    return [[0.5, 0.0, 0.0, 1.5, 2.0], [-1.0, 1.0, 0.5, 1.0, 1.0]]


def chain_known(nm, seed=3):
    """The first rows of the molecules fixed (3, 2, none, 2), known positions around KNOWN_CENTRE (tests/test_gpu_restraint_frame.py)."""
    Bn, N = nm.shape[:2]
    fm = torch.zeros(Bn, N, 1, dtype=torch.bool)
    for b, kf in enumerate((3, 2, 0, 2)[:Bn]):
        fm[b, :kf] = True
    fm &= nm
    g = torch.Generator().manual_seed(seed)
    xk = (torch.tensor(KNOWN_CENTRE) + torch.randn(Bn, N, 3, generator=g)) * fm
    hk = torch.randn(Bn, N, 8, generator=g) * fm
    return fm, xk.contiguous(), hk.contiguous()


def unnormalize(xh, nm, nv0, nv1, nb1):
    out = xh.double().clone()
    out[:, :, :3] *= nv0
    out[:, :, 3:] = out[:, :, 3:] * nv1 + nb1
    return out * nm.double()


_CHAINS = {}


def chain_reference(kind, precision):
    """The float64 restatement of one chain over the oracle (cached): a dict with the inputs of the device call (z, nm, em, ctx, raws,
    rs, ...), `states` (fp32, one per transition), `plain` (the last state of the same chain without the feature term), `calls` /
    `active` (network calls behind which the update ran / in which the feature term changed eps^) and, kind by kind, `frames` (the
    data predictions of record="x0", data units), `infos` / `state` (steering)."""
    key = (kind, precision)
    if key in _CHAINS:
        return _CHAINS[key]
    from hierdiff_amd import _lib, paths
    from hierdiff_amd.restraints import Restraints, feature_ratio
    from oracle import egnn_oracle as orc
    from tests import edit_reference as er
    from tests import guidance_reference as gr
    from tests import restraint_frame_reference as rf
    from tests import restraint_reference as rr
    from tests import sde_solver_reference as sd
    from tests import steer_reference as st
    from tests.test_inpaint_cpu import SEED, gamma_grid_fp64
    guided = "guided" in kind
    C_ = 1 if guided else 0
    H, L = CHAIN_SHAPES[precision]
    sd_np, cfg = er.weights(H, L, C_=C_)
    model = er.cpu_diffusion(sd_np, H, L, CHAIN_T, C_)
    gg = gamma_grid_fp64(model, CHAIN_T)
    path = paths.build_path(CHAIN_T, CHAIN_K)
    nv0, nv1, nb1 = CHAIN_NORM[0][0], CHAIN_NORM[0][1], CHAIN_NORM[1][1]
    ratio = feature_ratio("score", nv0, nv1)
    rows = rr.rows_from_grid(gg, path, "score", CHAIN_CLIP, nv0)
    mols = (6, 6, 6, 6) if kind == "steered" else CHAIN_MOLS
    _, _, nm, em, ctx = er.molecules(list(mols), C_=C_)
    Bn, N = nm.shape[:2]
    ft = chain_features()
    rs = Restraints(obstacles=chain_obstacles() if guided else None, features=ft)
    scale = torch.zeros(1) if kind == "steered" else torch.tensor(CHAIN_SCALE)
    net = er.RefNet(sd_np, cfg, CHAIN_T, nm, em, ctx)
    inner = gr.GuidedNet(net, er.RefNet(sd_np, cfg, CHAIN_T, nm, em, gr.null_ctx(nm)), 2.0, 0.0) if guided else net
    pos = rr.RestrainedNet(inner, rs, scale, rows, nv0) if guided else inner       # the position update of the obstacles
    pos_off = rr.RestrainedNet(inner, rs, scale, rows, nv0) if guided else inner
    fnet = FeatNet(pos, ft, scale, rows, nv1, nb1, ratio, nm=nm)
    off = FeatNet(pos_off, ft, torch.zeros(Bn), rows, nv1, nb1, ratio, nm=nm)
    out = dict(kind=kind, precision=precision, nm=nm, em=em, ctx=ctx, rs=rs, scale=scale, path=path, norm=CHAIN_NORM, guided=guided)
    if kind.startswith("inpaint"):
        R = int(kind[-1])
        lib = _lib.load()
        fm, xk, hk = chain_known(nm)
        ids = [INPAINT_BASE + b for b in range(Bn)]
        hk_n = (hk - nb1) / nv1
        xh_known = torch.cat([xk / nv0, hk_n], dim=2) * fm.float()
        z = orc.combined_noise(*rf.philox_raw(lib, SEED, ids, 0, N), nm.float())
        out.update(z=z, fm=fm, xk=xk, hk=hk, R=R,
                   states=rf.inpaint_path_ref(lib, fnet, gg, path, CHAIN_T, z, nm, fm, xh_known, R, SEED, ids),
                   plain=rf.inpaint_path_ref(lib, off, gg, path, CHAIN_T, z, nm, fm, xh_known, R, SEED, ids)[-1])
    elif kind == "steered":
        keep_total, keep_stage = st.energy_total, st.stage
        holder = {}

        def stage(rs_, z_, eps_, nm_, row3, nv0_, *a, **kw):
            holder["v"] = v_f32(z_, eps_, float(np.float32(row3[0])), float(np.float32(row3[1])), nv1, nb1).numpy()
            holder["va"] = v_mag(z_, eps_, float(np.float32(row3[0])), float(np.float32(row3[1])), nv1, nb1)
            return keep_stage(rs_, z_, eps_, nm_, row3, nv0_, *a, **kw)

        def energy_total(rs_, x0, nm_):
            U, mag = keep_total(rs_, x0, nm_)
            with np.errstate(all="ignore"):
                Uf = feature_energy_grad(ft, holder["v"], nm_)[0]
            uf = Uf[:, 0] + Uf[:, 1]
            return U + uf, mag + uf                           # (every term of U_feat is >= 0)

        st.energy_total, st.stage = energy_total, stage
        try:
            raw = st.normals_host(STEER_SEED, STEER_BASE, 0, Bn, N, 8)
            z = orc.combined_noise(raw[0], raw[1], nm.float()).float()
            snet = st.SteeredNet(fnet, rs, gg, path, STEER_BETA, STEER_P, STEER_RHO, STEER_SEED, STEER_BASE, CHAIN_T, 8, nv0)
            states, infos, state = snet.run(z, 1.0)
        finally:
            st.energy_total, st.stage = keep_total, keep_stage
        out.update(z=z, states=states, infos=infos, state=state, plain=None)
    else:
        raws = er.raw_draws(CHAIN_K + 2, Bn, N, seed=CHAIN_K)
        z = orc.combined_noise(raws[0][0], raws[0][1], nm.float())
        out.update(z=z, raws=raws)
        if kind == "sde2m":
            out["states"] = [r[0] for r in sd.chain_ref(fnet.net, gg, path, z, nm.float(), raws[1:])]
            out["plain"] = [r[0] for r in sd.chain_ref(off.net, gg, path, z, nm.float(), raws[1:])][-1]
        else:
            def run(n, frames=None):
                zz, states = z, []
                for k, (t, s) in enumerate(zip(path[:-1], path[1:])):
                    eps = n.net(zz, t)
                    if frames is not None:
                        al, sg = rows[int(t)][0], rows[int(t)][1]
                        frames.append(unnormalize((zz.double() - sg * eps.double()) / al, nm, nv0, nv1, nb1))
                    zz = gr.ancestral_on_eps(n.c, zz, eps, s, t, raws[1 + k], gg).float()
                    states.append(zz)
                return states
            frames = [] if kind == "x0" else None
            out["states"], out["plain"] = run(fnet, frames), run(off)[-1]
            out["frames"] = frames
    out.update(calls=fnet.calls, active=fnet.active)
    _CHAINS[key] = out
    return out
