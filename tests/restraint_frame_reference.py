"""Float64 restatement of restraints in the known fragments' frame (hd_restraint_frame 1 / hd_restrain_eps_framed /
hd_restraint_energy_framed and the restrained inpainting path loop; formulas in include/hierdiff_hip.h, "THE KNOWN FRAGMENTS'
FRAME"), the yardstick of tests/test_restraint_frame_cpu.py and tests/test_gpu_restraint_frame.py.

Molecule b at a transition with the row {alpha_t, sigma_t, lambda_k, clip_k}; x^0 the fp32 data prediction of the plain update
(`x0_f32`), F its valid fixed nodes, nf = |F|, xk = nv0 known_z as uploaded (NOT centred):

    tau   = mean_F(x^0) - mean_F(xk)                         nf = 0: tau = 0 and every node is free (the plain update)
    U     = the three energies with u = x^0_i - (y + tau) for obstacles and anchors; pairs do not see tau
    g_i   = dU/dx_i with tau held constant, FREE valid nodes only; a fixed node's gradient is 0 by definition - the block is the
            frame, and its own clashes are the user's input.  A pair between a free and a fixed node acts on the free node.
    d_i   = clip(s_b lambda_k g_i), 0 for fixed nodes
    m     = mean of d over ALL valid nodes
    eps^_x,i += d_i - m for every valid node (fixed nodes receive -m)

eps^_x stays mean-free, as the chain requires.  Behind the posterior step and the replacement (`replace_ref`), which puts the block
where the generated fixed rows' centre went, a free node has moved relative to the block by exactly its own d_i times the step's
coefficient on eps^: the common -m moves block and free nodes alike and drops out.  That is the point of the construction.

Everything is written on top of tests/restraint_reference.py: the energy and its gradient are evaluated on x^0 - tau (the same
function, translated arguments), the gradient of fixed nodes is then set to 0, and `project_step` does the rest.  MAGNITUDES follow
that module's rule (every term replaced by its absolute value, differences expanded); an obstacle or anchor offset
x^0_i - y - tau counts |x^0_i| + |y| + |mean_F x^0| + |mean_F xk|, the last two with the means of the absolute values."""
import numpy as np
import torch

from tests.restraint_reference import energy_grad, project_step, random_tables, rows_from_grid, x0_f32  # noqa: F401  (re-exported)
from tests.test_inpaint_cpu import philox_raw, replace_ref  # noqa: F401


def _masks(nm, fm, B, N):
    nm = np.asarray(nm).reshape(B, N) != 0
    return nm, (np.asarray(fm).reshape(B, N) != 0) & nm


def frame_shift_ref(x, xk, nm, fm, xa=None):
    """tau [B,3] = mean_F(x) - mean_F(xk) in float64 (0 without valid fixed nodes), and its magnitude mean_F|x| + mean_F|xk|
    (`xa`: the magnitude of x itself, default |x|)."""
    x, xk = np.asarray(x, dtype=np.float64), np.asarray(xk, dtype=np.float64)
    B, N = x.shape[:2]
    xa = np.abs(x) if xa is None else np.asarray(xa, dtype=np.float64)
    _, f = _masks(nm, fm, B, N)
    tau, mag = np.zeros((B, 3)), np.zeros((B, 3))
    for b in range(B):
        nf = int(f[b].sum())
        if nf:
            tau[b] = x[b][f[b]].sum(0) / nf - xk[b][f[b]].sum(0) / nf
            mag[b] = xa[b][f[b]].sum(0) / nf + np.abs(xk[b][f[b]]).sum(0) / nf
    return tau, mag


def _only(rs, pairs):
    """The tables of `rs` with the pair rows alone (`pairs`) or the obstacle and anchor rows alone."""
    out = object.__new__(type(rs))
    for k in ("obs", "pair_idx", "pair_f", "anc_idx", "anc_f"):
        t = getattr(rs, k)
        keep = k.startswith("pair") == bool(pairs)
        setattr(out, k, t if keep else t[:1, :0])
    return out


def framed_energy_grad(rs, x, xk, nm, fm, xa=None):
    """U [B,3], its magnitude, g [B,N,3] (free valid nodes; 0 on fixed ones), the magnitude of g, and tau [B,3], for positions x
    and known positions xk in data units."""
    x = np.asarray(x, dtype=np.float64)
    B, N = x.shape[:2]
    xa = np.abs(x) if xa is None else np.asarray(xa, dtype=np.float64)
    nmb, f = _masks(nm, fm, B, N)
    tau, tmag = frame_shift_ref(x, xk, nm, fm, xa)
    # translating the nodes by -tau is translating the obstacle and anchor centres by +tau (their magnitudes count tau's); pairs see
    # differences of nodes only, and neither tau nor its magnitude
    U, Um, g, ga = energy_grad(_only(rs, False), x - tau[:, None, :], nmb, xa + tmag[:, None, :])
    Up, Upm, gp, gpa = energy_grad(_only(rs, True), x, nmb, xa)
    U, Um, g, ga = U + Up, Um + Upm, g + gp, ga + gpa
    g[f] = 0.0
    ga[f] = 0.0
    return U, Um, g, ga, tau


def framed_grad(rs, z, eps, nm, fm, known, alpha, sigma, nv0, x0=None):
    """(g, ga) of `framed_energy_grad` on the fp32 data prediction of (z, eps) - the part of the update that does not depend on the
    scale, lambda or the clip.  `x0`: another fp32 evaluation of the data prediction (default: `x0_f32`)."""
    al, sg = float(np.float32(alpha)), float(np.float32(sigma))
    x0 = x0_f32(z, eps, al, sg, nv0).numpy() if x0 is None else np.asarray(x0)
    xa = (np.abs(z[:, :, :3].double().numpy()) + sg * np.abs(eps[:, :, :3].double().numpy())) * (nv0 / al)
    xk = float(np.float32(nv0)) * torch.as_tensor(known)[:, :, :3].double().numpy()
    _, _, g, ga, _ = framed_energy_grad(rs, x0, xk, nm, fm, xa)
    return g, ga


def restrain_framed_ref(rs, z, eps, nm, fm, known, scale, row4, nv0, x0=None, grad=None):
    """The framed update of one transition: (out [B,N,D] float64, magnitude [B,N,D], active [B] - whether any step is non-zero).
    known [B,N,D]: the uploaded normalised known values; row4, scale: as `restraint_reference.restrain_ref`.  `grad`: the
    `framed_grad` of the same inputs, where the caller has it."""
    B, N, D = eps.shape
    al, sg, lam, clip = (float(np.float32(v)) for v in row4)
    s = np.asarray(torch.as_tensor(scale, dtype=torch.float32).reshape(-1).numpy(), dtype=np.float64)
    s = np.broadcast_to(s, (B,)) if s.size == 1 else s
    g, ga = framed_grad(rs, z, eps, nm, fm, known, al, sg, nv0, x0) if grad is None else grad
    d, da = project_step(g, ga, np.asarray(nm).reshape(B, N), s * lam, clip)
    out = eps.detach().double().numpy().copy()
    mag = np.abs(out)
    out[:, :, :3] += d
    mag[:, :, :3] += da
    return out, mag, np.abs(d).reshape(B, -1).max(1) > 0


class FramedNet:
    """eps^ of a network call behind the framed update: `inner` has .net(z, t_idx); `rows` maps the grid index of a transition's
    departure level to its row.  Counts the calls in which the update moved eps^ (`active`) and all restrained calls (`calls`)."""

    def __init__(self, inner, rs, scale, rows, nm, fm, known, nv0=1.0):
        self.inner, self.rs, self.scale, self.rows, self.nv0 = inner, rs, scale, dict(rows), float(nv0)
        self.nm, self.fm, self.known, self.dtype = nm, fm, known, inner.dtype
        self.c = getattr(inner, "c", inner)
        self.active = self.calls = 0

    def net(self, z, t_idx):
        eps = self.inner.net(z, t_idx)
        if int(t_idx) not in self.rows:
            return eps
        out, _, act = restrain_framed_ref(self.rs, z, eps, self.nm, self.fm, self.known, self.scale, self.rows[int(t_idx)], self.nv0)
        self.calls += 1
        self.active += int(act.any())
        return torch.from_numpy(out).to(self.dtype)


def inpaint_path_ref(lib, fnet, gg, path, T, z, nm, fm, xh_known, R, seed, ids, k_lo=0, k_hi=None, x0_frames=None):
    """Transitions k_lo .. k_hi - 1 of the inpainting chain on the descending `path`, every round's eps^ from `fnet.net` (guided and
    restrained as `fnet` is), normals from the host twin of the generator in the documented draw layout
    draw = (T + 2) (3 j + k) + (T - s).  Returns the list of states (fp32) behind every transition; `x0_frames`: a list that receives
    (z, eps^) of every transition's last round."""
    from oracle import egnn_oracle as orc
    from tests import guidance_reference as gr
    nmf, fmf = nm.float(), fm.float()
    B, N = nmf.shape[:2]
    g32 = torch.as_tensor(gg, dtype=torch.float32).view(-1)
    K = len(path) - 1
    states = []
    for k in range(k_lo, K if k_hi is None else k_hi):
        t, s = path[k], path[k + 1]
        gs, gt = g32[s].expand(B, 1), g32[t].expand(B, 1)
        _, sigma_ts, alpha_ts = orc.sigma_and_alpha_t_given_s(gt, gs)
        alpha_s = torch.sqrt(torch.sigmoid(-gs)).view(-1, 1, 1)
        sigma_s = torch.sqrt(torch.sigmoid(gs)).view(-1, 1, 1)
        for j in range(R):
            draw = lambda kk: (T + 2) * (3 * j + kk) + (T - s)
            eps = fnet.net(z, t)
            if x0_frames is not None and j == R - 1:
                x0_frames.append((z.clone(), eps.clone()))
            z = gr.ancestral_on_eps(fnet.c, z, eps, s, t, philox_raw(lib, seed, ids, draw(0), N), g32).float()
            z = replace_ref(z, xh_known, nmf, fmf, alpha_s, sigma_s, philox_raw(lib, seed, ids, draw(1), N))
            if j < R - 1:
                e = orc.combined_noise(*philox_raw(lib, seed, ids, draw(2), N), nmf)
                z = alpha_ts.view(-1, 1, 1) * z + sigma_ts.view(-1, 1, 1) * e
        states.append(z)
    return states


# ----------------------------------------------------------------------------- the shared cases

CENTRE = (12.0, -7.0, 30.0)            # where the known fragments (and the tables around them) sit, data units: far from the origin
PQA = [(P, Q, A) for P in (0, 1, 7, 70) for Q in (0, 3) for A in (0, 2)]      # the grid of tests/test_gpu_restraint.py


def framed_tables(B, N, P, Q, A, seed, per_molecule, centre=CENTRE):
    """`random_tables` with the obstacle and anchor centres translated to `centre` (in fp32, as the tables are kept)."""
    rs, _ = random_tables(B, N, P, Q, A, seed, per_molecule)
    c = torch.tensor(centre, dtype=torch.float32)
    rs.obs = rs.obs.clone()
    rs.anc_f = rs.anc_f.clone()
    rs.obs[..., :3] += c
    rs.anc_f[..., :3] += c
    return rs


class _Case:
    pass


def kernel_case(N, D, nv0=1.7):
    """The five molecules of the kernel test: some fixed nodes; no fixed node; every valid node fixed; partly masked with fixed bytes
    among the masked rows (they must be ignored); one valid node (free).  z and eps hold values on masked rows too."""
    c = _Case()
    c.B, c.N, c.D, c.nv0 = 5, N, D, nv0
    h = (N + 1) // 2
    nm = torch.zeros(5, N, dtype=torch.bool)
    for b, n in enumerate((N, N, h, h, 1)):
        nm[b, :n] = True
    fm = torch.zeros(5, N, dtype=torch.bool)
    fm[0, 1:1 + max(2, N // 3)] = True
    fm[2, :h] = True
    fm[3, 0] = True
    fm[3, h - 1:] = True                                     # the last valid node and every masked row
    g = torch.Generator().manual_seed(N * 100 + D)
    c.z, c.eps = torch.randn(5, N, D, generator=g), torch.randn(5, N, D, generator=g)
    xk = torch.tensor(CENTRE) + torch.randn(5, N, 3, generator=g) * 1.5
    c.x_known = xk.contiguous()
    c.known = torch.randn(5, N, D, generator=g)               # feature columns and rows outside F: never read
    c.known[:, :, :3] = xk / nv0
    c.nm, c.fm = nm, fm
    c.scale = torch.tensor([1.0, 0.5, 2.0, 1.5, 1.0])
    return c
