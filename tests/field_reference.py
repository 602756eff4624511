"""Float64 restatement of the field restraints (hd_restraint_fields / hd_restraint_field_energy[_framed] and the field term of
hd_restrain_eps[_framed]; formulas in include/hierdiff_hip.h, "Field restraints"), the yardstick of tests/test_field_cpu.py and
tests/test_gpu_field.py.

Written from the formulas with plain Python loops over molecules, nodes, fields and the 8 corners: a hand-derived gradient, nothing
imported from the product but the `Field` / `Restraints` containers that hold the lattices.  For a valid node at x, p = x - tau:

    u_c = (p_c - o_c) / h_c,  ub_c = min(max(u_c, 0), n_c - 1),  cell_c = min(floor(ub_c), n_c - 2),  t_c = ub_c - cell_c
    V = sum_{a,b,c} v[cell + (a,b,c)] W_a(t_0) W_b(t_1) W_c(t_2),  out_c = (u_c - ub_c) h_c
    E = k w_i (V + 1/2 wall |out|^2),   dE/dx_c = k w_i ([0 <= u_c <= n_c - 1] dV/dt_c / h_c + wall out_c)

MAGNITUDES follow tests/restraint_reference.py: the same formula with every term replaced by its absolute value and every difference
expanded - t counts (|x| + |tau| + |o|) / h + cell where the coordinate is inside the box (exactly |ub| + cell where it is clamped),
1 - t counts 1 + that, out counts (|u| + |ub|) h.  The other restraint terms, the projection and the frame come from
tests/restraint_reference.py and tests/restraint_frame_reference.py unchanged.

MUTANTS: `mutant=` names one deliberate mistake in the restatement; tests/test_field_cpu.py asserts that each of them misses the GPU
bars on the inputs of the kernel test (`kernel_cases`), so the bars and the inputs can tell them from the truth."""
import contextlib
import functools
import math

import numpy as np
import torch

from tests import restraint_frame_reference as rf
from tests import restraint_reference as rr

MUTANTS = ("swap_axes", "no_inv_h", "no_clamp", "no_cap", "no_wall", "no_weights", "tau_sign")


def node_weights(f, b, N):
    """[N] float64: weights[i] of molecule b for i < W, 0 behind; None: ones."""
    if f.weights is None:
        return np.ones(N)
    w = np.asarray(f.weights.numpy(), dtype=np.float64)
    row = w[0 if w.shape[0] == 1 else b]
    out = np.zeros(N)
    n = min(N, row.shape[0])
    out[:n] = row[:n]
    return out


def field_node(f, p, pa, mutant=None):
    """One field at p [3] (magnitude pa [3]), without the factor k w_i: (e, |e|, g [3], |g| [3]), or None for a non-finite p."""
    p, pa = np.asarray(p, dtype=np.float64), np.asarray(pa, dtype=np.float64)
    if not np.isfinite(p).all():
        return None
    v = np.asarray(f.values.numpy(), dtype=np.float64)
    n = np.array(v.shape)
    o, h = np.asarray(f.origin.numpy(), dtype=np.float64), np.asarray(f.spacing.numpy(), dtype=np.float64)
    wall = 0.0 if mutant == "no_wall" else float(f.wall)
    top = n - 1.0
    u, um = (p - o) / h, (pa + np.abs(o)) / h
    inside = (u >= 0) & (u <= top)
    clamped = np.minimum(np.maximum(u, 0.0), top)
    if mutant == "no_clamp":
        ub, ubm, inside = u, um, np.ones(3, dtype=bool)
    else:
        ub, ubm = clamped, np.where(inside, um, np.abs(clamped))
    fl = np.floor(clamped).astype(np.int64)
    cell = fl if mutant == "no_cap" else np.minimum(fl, n - 2)
    t, tm = ub - cell, ubm + cell
    W = [(1.0 - t[c], t[c]) for c in range(3)]
    Wm = [(1.0 + tm[c], tm[c]) for c in range(3)]
    V = Va = 0.0
    d, da = np.zeros(3), np.zeros(3)
    for a in (0, 1):
        for b in (0, 1):
            for c in (0, 1):
                i0, i1, i2 = cell[0] + a, cell[1] + b, cell[2] + c
                if mutant == "swap_axes":                       # first and last axis swapped in the index, the strides kept
                    val = v.reshape(-1)[((i2 * n[1] + i1) * n[2] + i0) % v.size]
                elif mutant == "no_cap":                        # (the read past the end: the last value again)
                    val = v[min(i0, n[0] - 1), min(i1, n[1] - 1), min(i2, n[2] - 1)]
                else:
                    val = v[i0, i1, i2]
                V += val * W[0][a] * W[1][b] * W[2][c]
                Va += abs(val) * Wm[0][a] * Wm[1][b] * Wm[2][c]
                d[0] += (val if a else -val) * W[1][b] * W[2][c]
                d[1] += (val if b else -val) * W[0][a] * W[2][c]
                d[2] += (val if c else -val) * W[0][a] * W[1][b]
                da[0] += abs(val) * Wm[1][b] * Wm[2][c]
                da[1] += abs(val) * Wm[0][a] * Wm[2][c]
                da[2] += abs(val) * Wm[0][a] * Wm[1][b]
    out, outm = (u - ub) * h, np.where(u == ub, 0.0, (um + ubm) * h)
    e = V + 0.5 * wall * float((out * out).sum())
    ea = Va + 0.5 * wall * float((outm * outm).sum())
    hh = np.ones(3) if mutant == "no_inv_h" else h
    g = np.where(inside, d / hh, 0.0) + wall * out
    ga = np.where(inside, da / hh, 0.0) + wall * outm
    return e, ea, g, ga


def field_energy_grad(rs, x, nm, tau=None, taum=None, xa=None, mutant=None):
    """U_fld [B], its magnitude, g [B,N,3] = dU_fld/dx over all valid nodes and the magnitude of g, for positions x [B,N,3] read at
    x - tau (tau [B,3], magnitude taum; None: 0)."""
    x = np.asarray(x, dtype=np.float64)
    B, N = x.shape[:2]
    xa = np.abs(x) if xa is None else np.asarray(xa, dtype=np.float64)
    nm = np.asarray(nm).reshape(B, N) != 0
    tau = np.zeros((B, 3)) if tau is None else np.asarray(tau, dtype=np.float64)
    taum = np.abs(tau) if taum is None else np.asarray(taum, dtype=np.float64)
    U, Um, g, ga = np.zeros(B), np.zeros(B), np.zeros((B, N, 3)), np.zeros((B, N, 3))
    for b in range(B):
        for f in rs.fields:
            w = np.ones(N) if mutant == "no_weights" else node_weights(f, b, N)
            for i in range(N):
                kw = float(f.k) * w[i]
                if not nm[b, i] or not kw > 0:
                    continue
                p = x[b, i] + tau[b] if mutant == "tau_sign" else x[b, i] - tau[b]
                got = field_node(f, p, xa[b, i] + taum[b], mutant)
                if got is None:
                    continue
                U[b] += kw * got[0]
                Um[b] += kw * got[1]
                g[b, i] += kw * got[2]
                ga[b, i] += kw * got[3]
    return U, Um, g, ga


def field_energy_framed(rs, x, xk, nm, fm, mutant=None):
    """(U_fld [B], magnitude, tau [B,3]) in the frame of the known positions xk: all valid nodes at x - tau."""
    tau, tmag = rf.frame_shift_ref(x, xk, nm, fm)
    U, Um, _, _ = field_energy_grad(rs, x, nm, tau, tmag, mutant=mutant)
    return U, Um, tau


def restrain_ref(rs, z, eps, nm, scale, row4, nv0, fm=None, known=None, mutant=None):
    """The update of one transition with the field term next to the three tables: (out [B,N,D] float64, magnitude).  fm / known
    [B,N,D] (normalised, as uploaded): the framed update.  The arguments of `restraint_reference.restrain_ref`."""
    B, N, D = eps.shape
    al, sg, lam, clip = (float(np.float32(v)) for v in row4)
    s = np.asarray(torch.as_tensor(scale, dtype=torch.float32).reshape(-1).numpy(), dtype=np.float64)
    s = np.broadcast_to(s, (B,)) if s.size == 1 else s
    x0 = rr.x0_f32(z, eps, al, sg, nv0).numpy()
    xa = (np.abs(z[:, :, :3].double().numpy()) + sg * np.abs(eps[:, :, :3].double().numpy())) * (nv0 / al)
    if fm is None:
        _, _, g, ga = rr.energy_grad(rs, x0, nm, xa)
        _, _, fg, fga = field_energy_grad(rs, x0, nm, xa=xa, mutant=mutant)
    else:
        xk = float(np.float32(nv0)) * torch.as_tensor(known)[:, :, :3].double().numpy()
        _, _, g, ga, _ = rf.framed_energy_grad(rs, x0, xk, nm, fm, xa)
        tau, tmag = rf.frame_shift_ref(x0, xk, nm, fm, xa)
        _, _, fg, fga = field_energy_grad(rs, x0, nm, tau, tmag, xa, mutant)
        fixed = (np.asarray(fm).reshape(B, N) != 0) & (np.asarray(nm).reshape(B, N) != 0)
        fg[fixed] = 0.0
        fga[fixed] = 0.0
    d, da = rr.project_step(g + fg, ga + fga, np.asarray(nm).reshape(B, N), s * lam, clip)
    out = eps.detach().double().numpy().copy()
    mag = np.abs(out)
    out[:, :, :3] += d
    mag[:, :, :3] += da
    return out, mag


class FieldNet:
    """eps^ of a network call behind the restraint update with fields, plain or framed (`fm`, `known`): the pattern of
    `restraint_reference.RestrainedNet` / `restraint_frame_reference.FramedNet`.  Counts the restrained calls and those in which the
    field term alone moved eps^ (`active`)."""

    def __init__(self, inner, rs, scale, rows, nv0=1.0, nm=None, fm=None, known=None):
        self.inner, self.rs, self.scale, self.rows, self.nv0 = inner, rs, scale, dict(rows), float(nv0)
        self.dtype, self.nm = inner.dtype, inner.nm if nm is None else nm
        self.fm, self.known = fm, known
        self.c = getattr(inner, "c", inner)
        self.bare = with_fields(rs, [])              # the tables without the fields
        self.active = self.calls = 0

    def net(self, z, t_idx):
        eps = self.inner.net(z, t_idx)
        if int(t_idx) not in self.rows:
            return eps
        row = self.rows[int(t_idx)]
        out, _ = restrain_ref(self.rs, z, eps, self.nm, self.scale, row, self.nv0, self.fm, self.known)
        off, _ = restrain_ref(self.bare, z, eps, self.nm, self.scale, row, self.nv0, self.fm, self.known)
        self.calls += 1
        self.active += int(np.abs(out - off).max() > 0)
        return torch.from_numpy(out).to(self.dtype)


# ----------------------------------------------------------------------------- the shared cases

CENTRE = rf.CENTRE
ROW = (0.8, 0.6, 0.75)                   # alpha_t, sigma_t, lambda_k of the kernel cases; nv0 = 1.7
NV0 = 1.7
PLANE_MARGIN = 1e-4                     # cell widths
SHAPES = ((2, 2, 2), (3, 4, 5))          # the cell is always 0; non-cubic, anisotropic


def make_fields(NF, B, N, seed, per_molecule, centre=(0.0, 0.0, 0.0), k=None, nudge=0.0):
    """NF fields alternating between the (2,2,2) lattice of spacing 4 and the (3,4,5) lattice of spacing (0.5, 1, 2), origins away from
    0 (and around `centre`), values of both signs, wall 0 on the even fields and > 0 on the odd ones; weights None / [W] with W < N
    and zeros / per molecule [B, N] with zeros, by turns.  `nudge` moves every origin (`kernel_cases` uses it to keep the nodes off the lattice planes)."""
    from hierdiff_amd.restraints import Field
    rng = np.random.Generator(np.random.PCG64(seed))
    out = []
    for f in range(NF):
        shape = SHAPES[(f + seed) % 2]
        if shape == (2, 2, 2):
            o, h = np.array([-2.25, -1.75, -2.5]) + rng.uniform(-0.2, 0.2, 3), 4.0
        else:
            o, h = np.array([-0.75, -1.25, -3.5]) + rng.uniform(-0.2, 0.2, 3), (0.5, 1.0, 2.0)
        o = o + np.asarray(centre) + nudge
        kind = f % 3
        if kind == 0 and not (per_molecule and f == 0):
            w = None
        elif per_molecule and kind != 1:
            w = rng.uniform(0.25, 2.0, (B, N))
            w[:, 1::4] = 0.0
        else:
            w = rng.uniform(0.25, 2.0, max(2, N - 2))
            w[::3] = 0.0
        out.append(Field(rng.normal(0.0, 1.0, shape), o.tolist(), h, k=float(rng.uniform(0.5, 2.0)) if k is None else k,
                         wall=0.0 if f % 2 == 0 else float(rng.uniform(0.5, 2.0)), weights=w))
    return out


def with_fields(rs, fields):
    """The tables of `rs` (or none) and `fields` in one Restraints."""
    from hierdiff_amd.restraints import Restraints
    out = Restraints(fields=fields)
    if rs is not None:
        for k in ("obs", "pair_idx", "pair_f", "anc_idx", "anc_f"):
            setattr(out, k, getattr(rs, k))
    return out


class _Case:
    pass


def masks_for(N):
    nm = torch.zeros(3, N, dtype=torch.bool)
    for b, n in enumerate((N, (N + 1) // 2, 1)):              # a full molecule, a partly masked one, one valid node
        nm[b, :n] = True
    return nm


def kernel_cases(N, D, framed):
    """The inputs of the kernel tests at one shape: cases with .rs, .z, .eps, .nm, .scale, .row (4 floats), .nv0, and for the framed
    kernel .fm, .known, .x_known.  Plain: B = 3 (full, partly masked, one valid node).  Framed: the five molecules of
    `restraint_frame_reference.kernel_case` (some / no / all nodes fixed, ...), the known fragments around CENTRE.
    NF in {1, 3, 8} x shared / per-molecule weights x alone / with P, Q, A > 0 x clip inf / finite."""
    if framed:
        base = rf.kernel_case(N, D, NV0)
    else:
        base = _Case()
        base.B, base.N, base.D, base.nv0 = 3, N, D, NV0
        base.nm = masks_for(N)
        g = torch.Generator().manual_seed(N * 100 + D)
        base.z, base.eps = torch.randn(3, N, D, generator=g), torch.randn(3, N, D, generator=g)
        base.scale = torch.tensor([1.0, 0.5, 2.0])
        base.fm = base.known = base.x_known = None
    B = base.B
    centre = CENTRE if framed else (0.0, 0.0, 0.0)
    for NF in (1, 3, 8):
        for per in (False, True):
            for pqa in ((0, 0, 0), (7, 3, 2)):
                for clip in (math.inf, 0.2):
                    c = _Case()
                    c.__dict__.update(base.__dict__)
                    seed = NF + 10 * int(per) + 100 * pqa[0]
                    tabs = None
                    if pqa[0]:
                        tabs = rf.framed_tables(B, N, *pqa, seed, per) if framed else rr.random_tables(B, N, *pqa, seed, per)[0]
                    c.row = ROW + (clip,)
                    # the device may contract z - sigma eps into one fma (tests/restraint_reference.py): its x^0 can differ by an
                    # fp32 ulp, 8e-6 cell widths at |x| < 64 and h = 0.5.  The origins are nudged until no node is that close to a plane.
                    for attempt in range(50):
                        c.rs = with_fields(tabs, make_fields(NF, B, N, seed, per, centre, nudge=0.0137 * attempt))
                        if plane_distance(c.rs, *data_prediction(c)) > PLANE_MARGIN:
                            break
                    else:
                        raise AssertionError("no origin keeps the nodes off the lattice planes")
                    c.name = f"NF={NF} {'rows' if per else 'shared'} PQA={pqa} clip={clip}"
                    yield c


def data_prediction(c):
    """(x [B,N,3] float64 in the fields' frame, i.e. x^0 - tau, valid [B,N]) of a kernel case."""
    x0 = rr.x0_f32(c.z, c.eps, c.row[0], c.row[1], c.nv0).numpy().astype(np.float64)
    if c.fm is not None:
        xk = float(np.float32(c.nv0)) * c.known[:, :, :3].double().numpy()
        x0 = x0 - rf.frame_shift_ref(x0, xk, c.nm, c.fm)[0][:, None, :]
    return x0, c.nm.numpy()


def plane_distance(rs, x, valid):
    """The smallest distance, in cell widths, of a valid node's coordinate from a lattice plane (the planes u = 0 .. n - 1)."""
    worst = math.inf
    for f in rs.fields:
        o, h = f.origin.double().numpy(), f.spacing.double().numpy()
        u = (x[valid] - o) / h
        for c in range(3):
            near = np.clip(np.round(u[:, c]), 0, f.values.shape[c] - 1)
            worst = min(worst, float(np.abs(u[:, c] - near).min()))
    return worst


def exact_case(framed=False):
    """The deliberately exact points: alpha = 1, sigma = 0, nv0 = 1 so that x^0 = z bit for bit; one (3,4,5) lattice with origin
    (-1, -2, -4) and spacing (0.5, 1, 2) - powers of two, every u exact.  Nodes: an interior lattice point; the upper corner; one
    outside each of the six faces; inside a cell; NaN.  Two fields on that lattice: wall 0 and wall 2.  One molecule, mean-free z is
    not required by the kernel."""
    from hierdiff_amd.restraints import Field
    c = _Case()
    v = (np.arange(60, dtype=np.float64).reshape(3, 4, 5) ** 1.5 % 7.0 - 3.0).astype(np.float32).astype(np.float64)   # as fp32 keeps them
    pts = [[-0.5, -1.0, -2.0],            # lattice point (1, 1, 1)
           [0.0, 1.0, 4.0],               # the upper corner (2, 3, 4)
           [-1.5, -0.5, 1.0], [0.5, -0.5, 1.0], [-0.75, -2.5, 1.0], [-0.75, 1.5, 1.0], [-0.75, -0.5, -5.0], [-0.75, -0.5, 5.0],
           [-0.75, -0.5, 1.0],            # inside cell (0, 1, 2): t = (0.5, 0.5, 0.5)
           [float("nan"), 0.0, 0.0]]
    N, D = len(pts), 4
    c.B, c.N, c.D, c.nv0 = 1, N, D, 1.0
    c.nm = torch.ones(1, N, dtype=torch.bool)
    c.z = torch.zeros(1, N, D)
    c.z[0, :, :3] = torch.tensor(pts)
    c.eps = torch.zeros(1, N, D)
    c.scale = torch.ones(1)
    c.row = (1.0, 0.0, 1.0, math.inf)
    c.fm = c.known = c.x_known = None
    c.values = v
    c.rs = with_fields(None, [Field(v, [-1.0, -2.0, -4.0], (0.5, 1.0, 2.0), k=1.0, wall=0.0),
                              Field(v, [-1.0, -2.0, -4.0], (0.5, 1.0, 2.0), k=0.5, wall=2.0)])
    c.name = "exact points"
    return c


# ----------------------------------------------------------------------------- the steered chain with fields
# tests/steer_reference.py weighs the particles on its module-level `energy_total`; `steering_on_the_total` swaps in the total with
# U_fld, ((U_obs + U_pair) + U_anc) + U_fld, for the length of a block, so that `SteeredNet` runs the fielded chain unchanged.

def energy_total(rs, x0, nm):
    """U [B] = ((U_obs + U_pair) + U_anc) + U_fld and its magnitude."""
    with np.errstate(all="ignore"):
        U, mag, _, _ = rr.energy_grad(rs, x0, nm)
        Uf, Ufm, _, _ = field_energy_grad(rs, x0, nm)
    return ((U[:, 0] + U[:, 1]) + U[:, 2]) + Uf, ((mag[:, 0] + mag[:, 1]) + mag[:, 2]) + Ufm


@contextlib.contextmanager
def steering_on_the_total():
    from tests import steer_reference as st
    keep = st.energy_total
    st.energy_total = energy_total
    try:
        yield st
    finally:
        st.energy_total = keep


STEER_BETA, STEER_BASE, STEER_SCALE = 0.005, 24, 0.05


def steer_fields():
    """Two lattices around the origin with walls: the energy grows with the distance from the box, as the far-out data predictions of
    the noisy levels need for weights that differ."""
    from hierdiff_amd.restraints import Field
    g = np.random.Generator(np.random.PCG64(5))
    return [Field(g.normal(0.0, 2.0, (4, 5, 3)), [-3.0, -2.5, -3.5], (2.0, 1.25, 3.5), k=1.5, wall=0.5),
            Field(g.normal(0.0, 2.0, (2, 2, 2)), [-4.0, -3.5, -4.5], 8.0, k=1.0, wall=0.25, weights=[1.0, 0.0, 2.0, 1.0, 1.0, 0.5, 1.0])]


@functools.lru_cache(maxsize=None)
def steered_reference(precision, eta=1.0, base=STEER_BASE, beta=STEER_BETA, dtype=torch.float32, seed=2022):
    """(states, infos, final State, z_T, masks) of the steered chain of tests/steer_reference.py's fixture (T = 8, G = 2 groups of
    P = 4) with fields only: the gradient update (scale STEER_SCALE, clip 0.3) and the weights both see the fields."""
    from hierdiff_amd import paths
    from hierdiff_amd.restraints import Restraints
    from oracle import egnn_oracle as orc
    from tests import edit_reference as er
    from tests.test_inpaint_cpu import gamma_grid_fp64
    with steering_on_the_total() as st:
        H, L = st.CHAIN_SHAPES[precision]
        sd_np, cfg = er.weights(H, L)
        x, h, nm, em, _ = er.molecules(list(st.CHAIN_MOLS))
        B, N = nm.shape[:2]
        model = er.cpu_diffusion(sd_np, H, L, st.CHAIN_T)
        gg = gamma_grid_fp64(model, st.CHAIN_T)
        path = paths.build_path(st.CHAIN_T, None)
        rs = Restraints(fields=steer_fields())
        net = er.RefNet(sd_np, cfg, st.CHAIN_T, nm, em, None, dtype=dtype)
        inner = FieldNet(net, rs, torch.tensor([STEER_SCALE]), rr.rows_from_grid(gg, path, "score", 0.3))
        raw = st.normals_host(seed, base, 0, B, N, 8)
        z = orc.combined_noise(raw[0], raw[1], nm.float()).float()
        snet = st.SteeredNet(inner, rs, gg, path, beta, st.CHAIN_P, st.CHAIN_RHO, seed, base, st.CHAIN_T, 8)
        states, infos, state = snet.run(z, eta)
    return states, infos, state, z, (nm, em)
