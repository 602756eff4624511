"""Float64 restatement of steered sampling (hd_steer_step / the steered path loop; formulas in include/hierdiff_hip.h, "Steered
sampling"), the yardstick of tests/test_steer_cpu.py and tests/test_gpu_steer.py.

Written from the formulas with plain Python loops: the energies come from tests/restraint_reference.py (`energy_grad`), the data
prediction from its `x0_f32`, and nothing is imported from the product but the `Restraints` container and the two host twins of the
counter-based generator (hd_philox_uniform_host, hd_philox_normal_host), which are tested on their own.

Resampling is a DISCRETE decision: an ancestor changes when a resampling point (u + j) / P * S crosses a prefix sum, and a group is
resampled or not as ESS / P crosses rho.  A comparison of ancestors is therefore meaningful only where the reference itself is far
from both kinds of boundary; every stage reports its two MARGINS (as fractions of S, and of P) and the fixtures are chosen, and
asserted on the CPU, to keep them above the bars the tests state."""
import ctypes as C
import functools
import math

import numpy as np
import torch

from tests import restraint_reference as rr

UNIFORM_INDEX = 0xfffffffe


def uniform_host(seed, sample, draw):
    from hierdiff_amd import _lib
    return float(_lib.load().hd_philox_uniform_host(C.c_uint64(int(seed)), C.c_uint64(int(sample)), C.c_uint32(int(draw)),
                                                    C.c_uint32(UNIFORM_INDEX)))


def normals_host(seed, base, draw, B, N, F):
    """(randn_x [B,N,3], randn_h [B,N,F]) of the rows base .. base + B - 1 at `draw`: the layout of the library's noise kernels (entry
    n * (3 + F) + c of sample base + b)."""
    from hierdiff_amd import _lib
    fn = _lib.load().hd_philox_normal_host
    D = 3 + F
    out = np.empty((B, N, D), dtype=np.float32)
    for b in range(B):
        for e in range(N * D):
            out[b, e // D, e % D] = fn(int(seed), int(base) + b, int(draw), e)
    t = torch.from_numpy(out)
    return t[:, :, :3].contiguous(), t[:, :, 3:].contiguous()


def repeat_tables(rs, P):
    """Restraints whose per-molecule tables hold every row P times in a row (group g -> rows g P .. g P + P - 1); shared stay shared."""
    from hierdiff_amd.restraints import Restraints
    out = object.__new__(Restraints)
    for k in ("obs", "pair_idx", "pair_f", "anc_idx", "anc_f"):
        t = getattr(rs, k)
        setattr(out, k, t if t.shape[0] == 1 else t.repeat_interleave(P, dim=0).contiguous())
    out._model = None
    return out


class State:
    """The steering state of a chain: logw, U_prev [B] float64, root [B], and per group (events, smallest ESS, all-zero events)."""

    def __init__(self, B, P):
        self.P = P
        self.logw, self.uprev = np.zeros(B), np.zeros(B)
        self.lwmag, self.umag = np.zeros(B), np.zeros(B)         # the sums of the absolute values of their terms
        self.root = np.arange(B) % P
        self.stats = np.tile(np.array([0.0, float(P), 0.0]), (B // P, 1))


def energy_total(rs, x0, nm):
    """U [B] = (U_obs + U_pair) + U_anc and its magnitude (the sum of the absolute values of its terms: all are >= 0)."""
    with np.errstate(all="ignore"):                              # a non-finite position: the energy is, the gradient is not looked at
        U, mag, _, _ = rr.energy_grad(rs, x0, nm)
    return (U[:, 0] + U[:, 1]) + U[:, 2], (mag[:, 0] + mag[:, 1]) + mag[:, 2]


def weigh(state, U, Umag, beta):
    """logw += -beta (U - U_prev), U_prev = U; a non-finite U or update is weight 0."""
    for b in range(U.shape[0]):
        with np.errstate(invalid="ignore", over="ignore"):
            dl = -beta * (U[b] - state.uprev[b])
        state.logw[b] = state.logw[b] + dl if (math.isfinite(U[b]) and math.isfinite(dl)) else -math.inf
        state.lwmag[b] += beta * (Umag[b] + state.umag[b])
        state.uprev[b], state.umag[b] = U[b], Umag[b]


def systematic(w, u):
    """Ancestors of the weights w [P] under the uniform u: anc[j] = the smallest i whose inclusive prefix sum (index order) exceeds
    (u + j) / P * S, never past the last row of positive weight; and the smallest distance of a resampling point from a prefix sum,
    as a fraction of S."""
    P = len(w)
    cum, s = np.empty(P), 0.0
    for i in range(P):
        s += w[i]
        cum[i] = s
    last = max(i for i in range(P) if w[i] > 0.0)
    anc, margin = [], math.inf
    for j in range(P):
        target = (u + float(j)) / float(P) * s
        i = 0
        while i < P and not cum[i] > target:
            i += 1
        anc.append(min(i, last))
        margin = min(margin, float(np.abs(cum - target).min() / s))
    return np.asarray(anc), margin


def resample_group(logw, u, rho):
    """One group: (anc [P] local indices or None when nothing moves, ESS or None for an all-zero group, margin of the resampling
    points, margin of ESS / P against rho, the normalised prefix sums)."""
    P = len(logw)
    m = max(logw)
    if not m > -math.inf:
        return None, None, math.inf, math.inf, None
    w = np.array([math.exp(v - m) for v in logw])
    s, s2 = 0.0, 0.0
    for i in range(P):
        s += w[i]
        s2 += w[i] * w[i]
    ess = s * s / s2
    m_ess = abs(ess / P - rho)
    cumn = np.cumsum(w) / s
    if not ess < rho * P:
        return None, ess, math.inf, m_ess, cumn
    anc, margin = systematic(w, u)
    return anc, ess, margin, m_ess, cumn


def stage(rs, z, eps, nm, row3, nv0, state, rho, seed, base, draw, uniforms=None):
    """The steering stage of one transition on torch tensors z, eps [B,N,D] (returned rewritten in the moved rows; dtype kept) and
    `state` (in place).  Returns (z, eps, info): info['anc'] [B] the source ROW of every row, 'U' / 'Umag' [B], 'margin' /
    'margin_ess' the smallest margins over the groups, 'resampled' [G] bool, 'cum' the groups' normalised prefix sums."""
    P = state.P
    B = z.shape[0]
    al, sg, beta = (float(np.float32(v)) for v in row3)
    x0 = rr.x0_f32(z, eps, al, sg, nv0).numpy()
    U, Umag = energy_total(rs, x0, nm)
    weigh(state, U, Umag, beta)
    anc_rows = np.arange(B)
    margin, margin_ess, res, cums = math.inf, math.inf, [], []
    for g in range(B // P):
        lo = g * P
        u = uniform_host(seed, base + lo, draw) if uniforms is None else uniforms[g]
        anc, ess, m1, m2, cumn = resample_group(state.logw[lo:lo + P], u, rho)
        cums.append(cumn)
        margin, margin_ess = min(margin, m1), min(margin_ess, m2)
        if ess is None:
            state.stats[g, 2] += 1
        else:
            state.stats[g, 1] = min(state.stats[g, 1], ess)
        res.append(anc is not None)
        if anc is None:
            continue
        state.stats[g, 0] += 1
        anc_rows[lo:lo + P] = lo + anc
        state.root[lo:lo + P] = state.root[lo + anc]
        state.logw[lo:lo + P] = 0.0
        state.lwmag[lo:lo + P] = 0.0
    state.uprev, state.umag = state.uprev[anc_rows], state.umag[anc_rows]
    idx = torch.from_numpy(anc_rows)
    info = dict(anc=anc_rows, U=U, Umag=Umag, margin=margin, margin_ess=margin_ess, resampled=np.asarray(res), cum=cums)
    return z[idx].clone(), eps[idx].clone(), info


def steer_rows(gg, path, beta, schedule=None):
    """{k: (alpha_t, sigma_t, beta_k)} as the fp32 values the kernel is given (tests/restraint_reference.rows_from_grid's alpha /
    sigma)."""
    base = rr.rows_from_grid(gg, path, "sigma")
    return [(base[int(t)][0], base[int(t)][1], float(np.float32(beta * (1.0 if schedule is None else schedule[k]))))
            for k, t in enumerate(path[:-1])]


class SteeredNet:
    """The steered chain over the oracle, in the manner of `RestrainedNet`: `inner` has .net(z, t) (a RefNet, or a RestrainedNet over
    one) and .c (the RefNet the masks come from).  `run` walks the path with the ancestral (eta = 1) or DDIM-family (0 < eta < 1)
    update and noise from the host twins; every state is rounded once to fp32 as the device loop keeps it."""

    def __init__(self, inner, rs, gg, path, beta, P, rho, seed, base, T, F, nv0=1.0, schedule=None):
        self.inner, self.rs, self.gg, self.path = inner, rs, gg, list(path)
        self.rows = steer_rows(gg, path, beta, schedule)
        self.P, self.rho, self.seed, self.base, self.T, self.F, self.nv0 = P, rho, seed, base, T, F, float(nv0)
        self.nm = inner.nm

    def run(self, z, eta, k_lo=0, k_hi=None, state=None):
        from tests import edit_reference as er
        from tests import guidance_reference as gr
        B, N = self.nm.shape[:2]
        state = State(B, self.P) if state is None else state
        nmd = self.nm.to(torch.float64)
        k_hi = len(self.path) - 1 if k_hi is None else k_hi
        states, infos = [], []
        for k in range(k_lo, k_hi):
            t, s = self.path[k], self.path[k + 1]
            eps = self.inner.net(z, t)
            draw = self.T - s
            z, eps, info = stage(self.rs, z, eps, self.nm, self.rows[k], self.nv0, state, self.rho, self.seed, self.base, draw)
            infos.append(info)
            raw = normals_host(self.seed, self.base, draw, B, N, self.F)
            if eta == 1.0:
                z = gr.ancestral_on_eps(self.inner.c, z, eps, s, t, raw, self.gg).float()
            else:
                a, b, c = er.down_row(float(self.gg[s]), float(self.gg[t]), eta)
                from oracle import egnn_oracle as orc
                zs = a * z.double() - b * er._centre_x(eps.double(), nmd) + c * orc.combined_noise(raw[0], raw[1], self.nm.float()).double()
                z = er._centre_x(zs, nmd).float()
            states.append(z)
        return states, infos, state


def cumulative_difference(infos_a, infos_b):
    """The largest difference of the groups' normalised prefix sums between two runs of the same chain, over the transitions up to
    (and including) the first at which their ancestors differ; and whether the ancestors agreed throughout."""
    worst, same = 0.0, True
    for a, b in zip(infos_a, infos_b):
        for ca, cb in zip(a["cum"], b["cum"]):
            if ca is not None and cb is not None:
                worst = max(worst, float(np.abs(ca - cb).max()))
        if not np.array_equal(a["anc"], b["anc"]):
            same = False
            break
    return worst, same


# ----------------------------------------------------------------------------- the fixtures of the kernel tests
# hd_steer_step on a bare handle: G = 2 groups, two consecutive stages per case (the second sees the U_prev and logw the first left).
# alpha = sigma = 1/2, nv0 = 2 and inputs on a 2^-8 grid make x^0 = 4 (z - eps / 2) EXACT in fp32 whether or not the compiler fuses the
# multiply into the subtraction, so the energies are held to the double bar.  Margins of every case are asserted in test_steer_cpu.py.
STEP_ROW = (0.5, 0.5)
STEP_NV0 = 2.0
STEP_SEED, STEP_BASE = 2022, 1000
MARGIN_BAR = 1e-9
STEP_SHAPES = [(3, 5, 4), (4, 33, 11), (64, 5, 11), (64, 33, 4), (4, 5, 11), (3, 33, 4)]          # (P, N, D)
STEP_KINDS = ["resample", "none", "nonfinite", "allzero"]


def step_case(P, N, D, kind, per_group):
    """dict(rs, nm [B,N] bool, stages=[(z, eps, row3, draw)], rho) of one case; B = 2 P."""
    G = 2
    B = G * P
    seed = 1000 * P + 10 * N + D + 7 * STEP_KINDS.index(kind) + int(per_group)
    g = torch.Generator().manual_seed(seed)
    nm = torch.zeros(B, N, dtype=torch.bool)
    nm[:P, :N] = True
    nm[P:, :(N + 1) // 2] = True                                   # group 1: a partly masked molecule
    base, _ = rr.random_tables(G, N, 7, 3, 2, seed=seed, per_molecule=per_group)
    from hierdiff_amd.restraints import Restraints
    # every group also holds an anchor on node 0, so that a non-finite position of node 0 has a non-finite energy
    extra = torch.tensor([[0.0, 0.25, -0.5, 0.75, 0.5, 1.0]], dtype=torch.float64)
    anc = torch.cat([base.anc_idx.unsqueeze(-1).double(), base.anc_f.double()], dim=2)
    anc = torch.cat([anc, extra.expand(anc.shape[0], 1, 6)], dim=1)
    prs = torch.cat([base.pair_idx.double(), base.pair_f.double()], dim=2)
    sq = (lambda t: t) if per_group else (lambda t: t[0])
    rs = repeat_tables(Restraints(sq(base.obs.double()), sq(prs), sq(anc)), P)
    q = lambda t: torch.round(t * 256.0) / 256.0
    stages = []
    betas = {"resample": (0.02, 1.0), "none": (0.01, 0.002), "nonfinite": (0.02, 1.0), "allzero": (0.02, 1.0)}[kind]
    for i, beta in enumerate(betas):
        z, eps = q(torch.randn(B, N, D, generator=g) * 0.4), q(torch.randn(B, N, D, generator=g) * 0.4)
        if kind == "nonfinite" and i == 1:
            z[1, 0, 0] = math.inf
        if kind == "allzero" and i == 1:
            z[P:, 0, 0] = math.inf
        stages.append((z, eps, STEP_ROW + (beta,), 3 + i))
    return dict(rs=rs, nm=nm, stages=stages, rho=0.5, P=P, kind=kind)


def step_cases():
    for (P, N, D) in STEP_SHAPES:
        for kind in STEP_KINDS:
            yield (P, N, D, kind, (P + N + STEP_KINDS.index(kind)) % 2 == 0)


def step_reference(case):
    """The reference run of a case: [(z, eps, info, state copy)] per stage."""
    import copy
    B = case["nm"].shape[0]
    state = State(B, case["P"])
    out = []
    for (z, eps, row3, draw) in case["stages"]:
        zz, ee, info = stage(case["rs"], z, eps, case["nm"], row3, STEP_NV0, state, case["rho"], STEP_SEED, STEP_BASE, draw)
        out.append((zz, ee, info, copy.deepcopy(state)))
    return out


# ----------------------------------------------------------------------------- the fixtures of the chain tests
# T = 8 on the identity path, G = 2 groups of P = 4 (7 and 4 nodes), the tables of tests/test_gpu_restraint.py, with and without the
# gradient update.  With synthetic weights the data prediction of the noisy levels is far out and the energies are of order 1e5, so
# beta = 1e-4 is what gives transitions with and without resampling.  The sample id base of the fixtures is one at which the
# reference is far from every boundary (asserted in test_steer_cpu.py against the reference's own fp32 noise, figures in
# EXPERIMENTS.md).
CHAIN_T, CHAIN_P, CHAIN_MOLS, CHAIN_RHO, CHAIN_BETA, CHAIN_BASE = 8, 4, (7, 7, 7, 7, 4, 4, 4, 4), 0.5, 1e-4, 24
CHAIN_SHAPES = {"fp32": (32, 2), "fp16x3": (128, 1)}
CHAIN_RKW = dict(restraint_scale=0.05, restraint_clip=0.3)
MARGIN_FACTOR = 100.0
CHAIN_CASES = [(p, e, r) for p in ("fp32", "fp16x3") for e in (1.0, 0.5) for r in (False, True)]


def chain_tables(N):
    from hierdiff_amd.restraints import Restraints
    return Restraints(obstacles=[[0.5, 0.0, 0.0, 1.5, 2.0], [-1.0, 1.0, 0.5, 1.0, 1.0]],
                      pairs=[[0, 1, 2.0, 2.5, 1.0], [2, 3, 0.0, 0.5, 1.0], [1, N + 3, 0.0, 1.0, 1.0]], anchors=[[0, 1.0, 1.0, 1.0, 0.25, 1.5]])


@functools.lru_cache(maxsize=None)
def chain_reference(precision, eta, restrained, base=CHAIN_BASE, dtype=torch.float32, seed=2022):
    """(states, infos, final State, z_T, masks) of the reference chain of a fixture with the oracle in `dtype`."""
    from tests import edit_reference as er
    from tests.test_inpaint_cpu import gamma_grid_fp64
    from hierdiff_amd import paths
    from oracle import egnn_oracle as orc
    H, L = CHAIN_SHAPES[precision]
    sd_np, cfg = er.weights(H, L)
    x, h, nm, em, _ = er.molecules(list(CHAIN_MOLS))
    B, N = nm.shape[:2]
    model = er.cpu_diffusion(sd_np, H, L, CHAIN_T)
    gg = gamma_grid_fp64(model, CHAIN_T)
    path = paths.build_path(CHAIN_T, None)
    F = x.shape[-1] + h.shape[-1] - 3 if h.dim() == 3 else 8
    rs = chain_tables(N)
    net = er.RefNet(sd_np, cfg, CHAIN_T, nm, em, None, dtype=dtype)
    inner = rr.RestrainedNet(net, rs, torch.tensor([CHAIN_RKW["restraint_scale"] if restrained else 0.0]),
                             rr.rows_from_grid(gg, path, "score", CHAIN_RKW["restraint_clip"]) if restrained else {})
    raw = normals_host(seed, base, 0, B, N, F)
    z = orc.combined_noise(raw[0], raw[1], nm.float()).float()
    snet = SteeredNet(inner, rs, gg, path, CHAIN_BETA, CHAIN_P, CHAIN_RHO, seed, base, CHAIN_T, F)
    states, infos, state = snet.run(z, eta)
    return states, infos, state, z, (nm, em)
