"""Float64 restatement of the template restraints (hd_restraint_templates / hd_restraint_template_energy and the template term of
hd_restrain_eps[_framed]; formulas in include/hierdiff_hip.h, "Template restraints"), the yardstick of tests/test_template_cpu.py and
tests/test_gpu_template.py.

Written from the formulas with plain loops over molecules, templates and rows; nothing imported from the product but the `Template`
/ `Restraints` containers that hold the rows.  The rotation comes from the SINGULAR VALUE DECOMPOSITION with the determinant
correction, S = U diag(s) V^T, R = U diag(1, 1, det(U V^T)) V^T - deliberately not the kernel's method (Horn's quaternions by Jacobi).
Over the active rows (0 <= i_m < N, node i_m valid, w_m > 0) of template t in molecule b:

    W = sum w,  c_x = sum w x_i / W,  c_y = sum w y / W,  S = sum w (x_i - c_x)(y - c_y)^T,  r_m = (x_i - c_x) - R (y_m - c_y)
    U = 1/2 k sum w |r|^2,  rmsd = sqrt(sum w |r|^2 / W),  dU/dx_i += k w r_m

W = 0, one active row or a non-finite active coordinate: nothing.  CONDITIONING: R is unique iff s_2 + d s_3 > 0, d = sign(det S);
`cond` = (s_2 + d s_3) / s_1 is returned with every fit, and the compared cases keep it >= COND_MIN (asserted on the CPU).

MAGNITUDES follow tests/restraint_reference.py: every term replaced by its absolute value, every difference expanded - r_m counts
|x_i| + sum w |x| / W + sum_j |R_cj| (|y_j| + sum w |y_j| / W), with |x| the magnitude `xa` of the data prediction's own terms.

THE KERNEL'S x^0.  The device may contract z - sigma eps into one fused multiply-add (tests/restraint_reference.py), and a rotation
is not a term-by-term function of x^0.  The kernel cases therefore use sigma_t = 0.5: sigma eps is then exact in fp32, the contracted
and the plain form round the same number, and `restraint_reference.x0_f32` IS the kernel's fp32 x^0, bit for bit.

MUTANTS: `mutant=` names one deliberate mistake; tests/test_template_cpu.py asserts that each of them misses the GPU bars on the
inputs of the kernel test (`kernel_cases`)."""
import contextlib
import functools
import math

import numpy as np
import torch

from tests import field_reference as fr
from tests import restraint_frame_reference as rf
from tests import restraint_reference as rr

MUTANTS = ("r_transposed", "no_det", "unweighted_centroids", "centroid_all_nodes", "no_w_in_grad", "no_k", "masked_rows")
COND_MIN = 0.05


def rows_of(t, b):
    """(idx [M] int, y [M,3], w [M]) float64 of template t in molecule b."""
    r = 0 if t.rows == 1 else b
    return (np.asarray(t.index[r].numpy(), dtype=np.int64), np.asarray(t.positions[r].numpy(), dtype=np.float64),
            np.asarray(t.weights[r].numpy(), dtype=np.float64))


def rotation_svd(S, mutant=None):
    """(R, cond) for S [3,3] = sum w x' y'^T."""
    U, s, Vt = np.linalg.svd(S)
    d = 1.0 if np.linalg.det(U @ Vt) >= 0 else -1.0
    R = U @ np.diag([1.0, 1.0, 1.0 if mutant == "no_det" else d]) @ Vt
    cond = (s[1] + d * s[2]) / s[0] if s[0] > 0 else 0.0
    return (R.T if mutant == "r_transposed" else R), cond


def fit_one(t, b, x, valid, xa=None, mutant=None):
    """The fit of template t in molecule b at x [N,3]: None when it contributes nothing, else a dict with R, cx, cy, W, rows (the active
    row numbers), r [rows,3], rm (its magnitude), q = sum w |r|^2, cond."""
    N = x.shape[0]
    idx, y, w = rows_of(t, b)
    xa = np.abs(x) if xa is None else xa
    act = [m for m in range(len(idx)) if 0 <= idx[m] < N and w[m] > 0 and (valid[idx[m]] or mutant == "masked_rows")]
    if len(act) < 2 or not np.isfinite(x[idx[act]]).all():
        return None
    i, ya, wa = idx[act], y[act], w[act]
    W = wa.sum()
    cw = np.ones_like(wa) if mutant == "unweighted_centroids" else wa
    if mutant == "centroid_all_nodes":
        cx, cxm = x[valid].mean(0), xa[valid].mean(0)
    else:
        cx, cxm = (cw[:, None] * x[i]).sum(0) / cw.sum(), (cw[:, None] * xa[i]).sum(0) / cw.sum()
    cy, cym = (cw[:, None] * ya).sum(0) / cw.sum(), (cw[:, None] * np.abs(ya)).sum(0) / cw.sum()
    xp, yp = x[i] - cx, ya - cy
    S = (wa[:, None, None] * xp[:, :, None] * yp[:, None, :]).sum(0)
    R, cond = rotation_svd(S, mutant) if t.fit == "rigid" else (np.eye(3), 1.0)
    r = xp - yp @ R.T
    rm = xa[i] + cxm + (np.abs(ya) + cym) @ np.abs(R).T
    return dict(R=R, cx=cx, cy=cy, W=W, rows=act, idx=i, w=wa, r=r, rm=rm, q=float((wa * (r * r).sum(1)).sum()), cond=cond)


def template_energy_grad(rs, x, nm, xa=None, mutant=None):
    """U [B,NT], its magnitude (equal: every term is >= 0), g [B,N,3] = dU_tpl/dx over all valid nodes, the magnitude of g, and the
    fits [B][NT] (None or the dict of `fit_one`)."""
    x = np.asarray(x, dtype=np.float64)
    B, N = x.shape[:2]
    xa = np.abs(x) if xa is None else np.asarray(xa, dtype=np.float64)
    nm = np.asarray(nm).reshape(B, N) != 0
    NT = len(rs.templates)
    U, g, ga, fits = np.zeros((B, NT)), np.zeros((B, N, 3)), np.zeros((B, N, 3)), []
    for b in range(B):
        fits.append([])
        for j, t in enumerate(rs.templates):
            f = fit_one(t, b, x[b], nm[b], xa[b], mutant)
            fits[b].append(f)
            if f is None:
                continue
            k = 1.0 if mutant == "no_k" else float(t.k)
            U[b, j] = 0.5 * k * f["q"]
            for m in range(len(f["rows"])):
                wm = 1.0 if mutant == "no_w_in_grad" else f["w"][m]
                g[b, f["idx"][m]] += k * wm * f["r"][m]
                ga[b, f["idx"][m]] += k * wm * f["rm"][m]
    return U, U.copy(), g, ga, fits


def fit16(f):
    """(R row-major, c_x, c_y, rmsd) of a fit, as hd_restraint_template_energy reports it; nothing: R = I, zeros."""
    if f is None:
        return np.concatenate([np.eye(3).reshape(9), np.zeros(7)])
    return np.concatenate([f["R"].reshape(9), f["cx"], f["cy"], [math.sqrt(f["q"] / f["W"])]])


def restrain_ref(rs, z, eps, nm, scale, row4, nv0, fm=None, known=None, mutant=None):
    """The update of one transition with the template term behind the tables and the fields: (out [B,N,D] float64, magnitude).
    fm / known [B,N,D] (normalised, as uploaded): the framed update.  The arguments of `field_reference.restrain_ref`."""
    B, N, D = eps.shape
    al, sg, lam, clip = (float(np.float32(v)) for v in row4)
    s = np.asarray(torch.as_tensor(scale, dtype=torch.float32).reshape(-1).numpy(), dtype=np.float64)
    s = np.broadcast_to(s, (B,)) if s.size == 1 else s
    x0 = rr.x0_f32(z, eps, al, sg, nv0).numpy()
    xa = (np.abs(z[:, :, :3].double().numpy()) + sg * np.abs(eps[:, :, :3].double().numpy())) * (nv0 / al)
    _, _, tg, tga, _ = template_energy_grad(rs, x0, nm, xa, mutant)          # a template never sees tau
    if fm is None:
        _, _, g, ga = rr.energy_grad(rs, x0, nm, xa)
        _, _, fg, fga = fr.field_energy_grad(rs, x0, nm, xa=xa)
    else:
        xk = float(np.float32(nv0)) * torch.as_tensor(known)[:, :, :3].double().numpy()
        _, _, g, ga, _ = rf.framed_energy_grad(rs, x0, xk, nm, fm, xa)
        tau, tmag = rf.frame_shift_ref(x0, xk, nm, fm, xa)
        _, _, fg, fga = fr.field_energy_grad(rs, x0, nm, tau, tmag, xa)
        fixed = (np.asarray(fm).reshape(B, N) != 0) & (np.asarray(nm).reshape(B, N) != 0)
        for a in (fg, fga, tg, tga):                                         # only free nodes gather
            a[fixed] = 0.0
    d, da = rr.project_step((g + fg) + tg, (ga + fga) + tga, np.asarray(nm).reshape(B, N), s * lam, clip)
    out = eps.detach().double().numpy().copy()
    mag = np.abs(out)
    out[:, :, :3] += d
    mag[:, :, :3] += da
    return out, mag


def with_templates(rs, templates):
    """The tables and fields of `rs` (or none) and `templates` in one Restraints."""
    from hierdiff_amd.restraints import Restraints
    out = Restraints(templates=templates)
    if rs is not None:
        for k in ("obs", "pair_idx", "pair_f", "anc_idx", "anc_f", "fields"):
            setattr(out, k, getattr(rs, k))
    return out


class TemplateNet:
    """eps^ of a network call behind the restraint update with templates, plain or framed (`fm`, `known`): the pattern of
    `field_reference.FieldNet`.  Counts the restrained calls and those in which the template term alone moved eps^ (`active`)."""

    def __init__(self, inner, rs, scale, rows, nv0=1.0, nm=None, fm=None, known=None):
        self.inner, self.rs, self.scale, self.rows, self.nv0 = inner, rs, scale, dict(rows), float(nv0)
        self.dtype, self.nm = inner.dtype, inner.nm if nm is None else nm
        self.fm, self.known = fm, known
        self.c = getattr(inner, "c", inner)
        self.bare = with_templates(rs, [])
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

ROW = (0.8, 0.5, 0.75)                  # alpha_t, sigma_t (a power of two: module docstring), lambda_k of the kernel cases
NV0 = 1.7
DEGENERATE = ("two rows", "collinear rows")          # compared in energy and finiteness only


class _Case:
    pass


def masks_for(N):
    nm = torch.zeros(5, N, dtype=torch.bool)
    for b, n in enumerate((N, (N + 1) // 2, 1, N, max(2, N - 2))):      # full, partly masked, one valid node, full, nearly full
        nm[b, :n] = True
    return nm


def base_case(N, D, framed):
    if framed:
        return rf.kernel_case(N, D, NV0)
    c = _Case()
    c.B, c.N, c.D, c.nv0 = 5, N, D, NV0
    c.nm = masks_for(N)
    g = torch.Generator().manual_seed(N * 100 + D)
    c.z, c.eps = torch.randn(5, N, D, generator=g), torch.randn(5, N, D, generator=g)
    c.scale = torch.tensor([1.0, 0.5, 2.0, 1.5, 1.0])
    c.fm = c.known = c.x_known = None
    return c


def data_prediction(c):
    return rr.x0_f32(c.z, c.eps, c.row[0], c.row[1], c.nv0).numpy().astype(np.float64)


def make_templates(NT, M, B, N, seed, per_molecule):
    """NT templates of M rows with random positions and weights; template 1 is a "translation" fit.  M = 3: the nodes 0, 1, 2 in a
    random order.  M >= 8: row 2 names node 0, the others random nodes 1 .. N - 1 (several rows on one node; row 1 names the node of
    row 0), the rows 3, 5 and 7 name node -1, a node >= N and carry w = 0.  Through the masks of the cases rows name masked nodes,
    and the one-node molecule keeps exactly one active row.  (Two active rows, or several rows on the only valid node, would make R
    ambiguous: those are the named degenerate cases' business.)"""
    from hierdiff_amd.restraints import Template
    rng = np.random.Generator(np.random.PCG64(seed))
    R = B if per_molecule else 1
    out = []
    for t in range(NT):
        idx = np.stack([rng.permutation(3)[:M] if M <= 3 else rng.integers(1, N, M) for _ in range(R)])
        y = rng.normal(0.0, 1.5, (R, M, 3)) + rng.normal(0.0, 3.0, 3)
        w = rng.uniform(0.25, 2.0, (R, M))
        if M >= 8:
            idx[:, 1], idx[:, 2] = idx[:, 0], 0
            idx[:, 3], idx[:, 5], w[:, 7] = -1, N + 1, 0.0
        sq = (lambda a: a) if per_molecule else (lambda a: a[0])
        out.append(Template(sq(idx), sq(y), sq(w), k=float(rng.uniform(0.5, 2.0)), fit="translation" if t == 1 else "rigid"))
    return out


def worst_cond(rs, x, nm):
    """The smallest conditioning measure over the fits that contribute (inf: none does)."""
    fits = template_energy_grad(rs, x, nm)[4]
    return min([f["cond"] for row in fits for f in row if f is not None] + [math.inf])


def _special(name, c, N):
    """The templates of a named case, built on the data prediction of molecule 0 (all N nodes valid there or, framed, in molecule 0)."""
    from hierdiff_amd.restraints import Template
    x0 = data_prediction(c)[0]
    rng = np.random.Generator(np.random.PCG64(len(name)))
    Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    Q = Q if np.linalg.det(Q) > 0 else -Q
    n4 = list(range(min(N, 5)))
    if name == "mirror image":                          # the arrangement itself, reflected: every pair distance fits, the chirality does not
        return [Template(n4, x0[n4] * np.array([1.0, 1.0, -1.0]) + 0.01 * rng.normal(size=(len(n4), 3)), k=1.5)]
    if name == "exact fit":                             # x = Q y + s up to the fp32 rounding of y
        return [Template(n4, (x0[n4] - np.array([1.0, -2.0, 0.5])) @ Q, k=2.0)]
    if name == "edge rows":                             # a usual template; one active row; none; every weight 0
        return [make_templates(1, 3, 5, N, 3, False)[0], Template([0, -1, N + 3], rng.normal(size=(3, 3))),
                Template([-1, -1, N], rng.normal(size=(3, 3))), Template([0, 1, 2], rng.normal(size=(3, 3)), weights=[0.0, 0.0, 0.0])]
    if name == "two rows":
        return [Template([0, 1], rng.normal(size=(2, 3)), k=1.5)]
    if name == "collinear rows":
        return [Template([0, 1, 2], np.outer([-1.0, 0.5, 2.0], [1.0, 2.0, -1.0]) + 0.5, k=1.5)]
    raise KeyError(name)


def kernel_cases(N, D, framed):
    """The inputs of the kernel tests at one shape: cases with .rs, .z, .eps, .nm, .scale, .row (4 floats), .nv0, .name, .degenerate and
    for the framed kernel .fm, .known, .x_known.  B = 5.  Plain: full / partly masked / one valid node / full / nearly full.  Framed:
    the five molecules of `restraint_frame_reference.kernel_case` (some / no / all nodes fixed, ...).
    The grid NT in {1, 2, 4} x M in {3, 20} x shared / per-molecule rows, alternating alone / with P, Q, A, NF > 0 and clip inf /
    finite so that every pair of settings occurs; then the named cases: far from the origin, a mirror image, an exact fit, the edge
    rows, and the two degenerate ones."""
    base = base_case(N, D, framed)
    B = base.B
    n = 0
    for NT in (1, 2, 4):
        for M in (3, 20):
            for per in (False, True):
                c = _Case()
                c.__dict__.update(base.__dict__)
                pqa = (7, 3, 2) if n % 2 else (0, 0, 0)
                clip = 0.2 if (n // 2 + n) % 2 else math.inf
                n += 1
                c.row = ROW + (clip,)
                tabs = None
                if pqa[0]:
                    tabs = rf.framed_tables(B, N, *pqa, n, per) if framed else rr.random_tables(B, N, *pqa, n, per)[0]
                    tabs = fr.with_fields(tabs, fr.make_fields(2, B, N, n, per, rf.CENTRE if framed else (0.0, 0.0, 0.0)))
                for attempt in range(400):                     # (a margin over COND_MIN: the assertion is not at the mercy of a rounding)
                    c.rs = with_templates(tabs, make_templates(NT, M, B, N, 1000 * attempt + 10 * n + NT, per))
                    if worst_cond(c.rs, data_prediction(c), c.nm.numpy()) >= 1.5 * COND_MIN:
                        break
                else:
                    raise AssertionError("no seed gives well-conditioned fits")
                c.name = f"NT={NT} M={M} {'rows' if per else 'shared'} PQA={pqa} clip={clip}"
                c.degenerate = False
                yield c
    for name in ("far from the origin", "mirror image", "exact fit", "edge rows") + DEGENERATE:
        c = _Case()
        c.__dict__.update(base.__dict__)
        c.row = ROW + (math.inf,)
        if name == "far from the origin":
            c.z = base.z.clone()
            c.z[:, :, :3] += torch.tensor([40.0, -25.0, 60.0])
            c.rs = with_templates(None, make_templates(2, 20, B, N, 77, True))
        else:
            c.rs = with_templates(None, _special(name, c, N))
        c.name, c.degenerate = name, name in DEGENERATE
        yield c


# ----------------------------------------------------------------------------- the steered chain with templates
# as tests/field_reference.py: `SteeredNet` weighs on the module-level `energy_total` of tests/steer_reference.py

def energy_total(rs, x0, nm):
    """U [B] = (((U_obs + U_pair) + U_anc) + U_fld) + U_tpl and its magnitude."""
    with np.errstate(all="ignore"):
        U3, m3 = rr.energy_grad(rs, x0, nm)[:2]
        U, mag = (U3[:, 0] + U3[:, 1]) + U3[:, 2], (m3[:, 0] + m3[:, 1]) + m3[:, 2]
        if rs.n_fields:
            Uf, Ufm = fr.field_energy_grad(rs, x0, nm)[:2]
            U, mag = U + Uf, mag + Ufm
        Ut = template_energy_grad(rs, x0, nm)[0]
    ut = np.zeros(Ut.shape[0])
    for j in range(Ut.shape[1]):
        ut = ut + Ut[:, j]
    return U + ut, mag + ut


@contextlib.contextmanager
def steering_on_the_total():
    from tests import steer_reference as st
    keep = st.energy_total
    st.energy_total = energy_total
    try:
        yield st
    finally:
        st.energy_total = keep


STEER_BETA, STEER_BASE, STEER_SCALE = 0.001, 24, 0.05


def steer_templates():
    """A rigid five-node arrangement and a translation-only triangle on other nodes."""
    from hierdiff_amd.restraints import Template
    g = np.random.Generator(np.random.PCG64(9))
    return [Template([0, 1, 2, 3, 4], g.normal(0.0, 1.5, (5, 3)), weights=[1.0, 2.0, 1.0, 0.5, 1.0], k=1.5),
            Template([1, 3, 5], g.normal(0.0, 1.5, (3, 3)) + 2.0, k=1.0, fit="translation")]


@functools.lru_cache(maxsize=None)
def steered_reference(precision, eta=1.0, base=STEER_BASE, beta=STEER_BETA, dtype=torch.float32, seed=2022):
    """(states, infos, final State, z_T, masks) of the steered chain of tests/steer_reference.py's fixture (T = 8, G = 2 groups of
    P = 4) with templates only: the gradient update (scale STEER_SCALE, clip 0.3) and the weights both see the templates."""
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
        rs = Restraints(templates=steer_templates())
        net = er.RefNet(sd_np, cfg, st.CHAIN_T, nm, em, None, dtype=dtype)
        inner = TemplateNet(net, rs, torch.tensor([STEER_SCALE]), rr.rows_from_grid(gg, path, "score", 0.3))
        raw = st.normals_host(seed, base, 0, B, N, 8)
        z = orc.combined_noise(raw[0], raw[1], nm.float()).float()
        snet = st.SteeredNet(inner, rs, gg, path, beta, st.CHAIN_P, st.CHAIN_RHO, seed, base, st.CHAIN_T, 8)
        states, infos, state = snet.run(z, eta)
    return states, infos, state, z, (nm, em)
