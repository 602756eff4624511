"""Restatement of partial inpainting (hd_inpaint_parts / hd_inpaint_replace / hd_inpaint_decode_fix_parts; algorithm in
include/hierdiff_hip.h, "PARTIAL INPAINTING"), the yardstick of tests/test_inpaint_parts_cpu.py and tests/test_gpu_inpaint_parts.py.

Two masks instead of one: fx [B,N,1] "the position of this node is known", fh [B,N,F] "this feature channel of this node is known".
`replace_parts_ref` is `tests.test_inpaint_cpu.replace_ref` with the element-wise mask in place of the node mask and the position
mask wherever the centre of gravity is concerned - the same torch operations in the same order, so that coinciding masks give
`replace_ref`'s bits.  It runs in the dtype of its arguments: float32 is the restatement the chains are held against, float64 the
reference of the kernel test.

THE BAR of the kernel test is the project's element-wise one (tests/sampling_reference.py): |got - ref| <= BOUND * 2^-23 * A with A
the sum of the absolute values of the terms of that element (`replace_parts_mag`):
    a feature element          replaced: |alpha known| + |sigma e|;  else |z_gen| (it keeps its bits)
    a position element, |Fx| > 0
        t = replaced: |alpha known| + |sigma e| + mean_Fx|z_gen.x| + mean_Fx(|alpha known| + |sigma e|);  else |z_gen|
        A = t + mean over the valid nodes of t                                       (the re-centring)
    a position element, |Fx| = 0   |z_gen| (it keeps its bits)

MUTANTS are wrong readings of the two masks a kernel could make; tests/test_inpaint_parts_cpu.py shows that each of them misses
the bar on the kernel test's inputs (`kernel_case`) by a wide factor, so the GPU test cannot pass with one of them."""
import numpy as np
import torch

from oracle import egnn_oracle as orc
from tests import sampling_reference as sref
from tests.test_inpaint_cpu import philox_raw  # noqa: F401  (re-exported)

MUTANTS = ("any_channel", "x_mask_for_h", "shift_over_h", "compact_normals", "transposed")
CENTRE = (12.0, -7.0, 30.0)            # where the known positions sit, data units
NV0 = 1.7
CHANNELS = (0, 3, 7)


def masks_of(nm, fx, fh, dtype):
    """(fx [B,N,1], fh [B,N,F], element mask [B,N,3+F]) as `dtype`, each cut to the node mask."""
    B, N = nm.shape[:2]
    nmb = nm.reshape(B, N, 1) != 0
    fxb = (fx.reshape(B, N, 1) != 0) & nmb
    fhb = (fh.reshape(B, N, -1) != 0) & nmb
    return fxb.to(dtype), fhb.to(dtype), torch.cat([fxb.expand(B, N, 3), fhb], dim=2).to(dtype)


def _mutate(fxf, fhf, mutant):
    """(element mask, mask of the nodes the shift runs over) under `mutant`."""
    B, N, F = fhf.shape
    sf = fxf
    if mutant == "any_channel":
        fhf = (fhf.sum(2, keepdim=True) > 0).to(fhf.dtype).expand(B, N, F)
    elif mutant == "x_mask_for_h":
        fhf = fxf.expand(B, N, F)
    elif mutant == "shift_over_h":
        sf = (fhf.sum(2, keepdim=True) > 0).to(fhf.dtype)
    elif mutant == "transposed":
        fhf = fhf.reshape(B, F, N).transpose(1, 2)
    return torch.cat([fxf.expand(B, N, 3), fhf], dim=2), sf


def replace_parts_ref(z_gen, xh_known, nm, fx, fh, alpha_s, sigma_s, raw, mutant=None):
    """Steps 2' - 3' on z_gen [B,N,D] in its own dtype.  nm [B,N,1], fx [B,N,1], fh [B,N,F] (any dtype, non-zero = set; bytes on
    masked rows are ignored); alpha_s / sigma_s: [B,1,1] tensors or numbers; raw = (raw_x [B,N,3], raw_h [B,N,F]), the normals of
    EVERY element at its own index e = n D + c."""
    dt = z_gen.dtype
    B, N, D = z_gen.shape
    nmf = (nm.reshape(B, N, 1) != 0).to(dt)
    fxf, fhf, em = masks_of(nm, fx, fh, dt)
    sf = fxf
    if mutant is not None:
        em, sf = _mutate(fxf, fhf, mutant)
        em = em * nmf                                        # (a mutant still skips the masked rows)
    e_all = torch.cat(raw, dim=2).to(dt)
    if mutant == "compact_normals":                          # the k-th replaced element of a molecule takes normal k
        flat, keep = e_all.reshape(B, N * D), em.reshape(B, N * D) != 0
        e_all = torch.zeros_like(flat)
        for b in range(B):
            e_all[b, keep[b]] = flat[b, :int(keep[b].sum())]
        e_all = e_all.reshape(B, N, D)
    xh_known = torch.where(em != 0, xh_known.to(dt), torch.zeros((), dtype=dt))      # garbage outside the masks is never read
    e_kn = e_all * em
    z_kn = (alpha_s * xh_known + sigma_s * e_kn) * em
    nfix = sf.sum(1, keepdim=True)
    has = nfix > 0
    den = torch.where(has, nfix, torch.ones_like(nfix))
    c = (z_gen[:, :, :3] * sf).sum(1, keepdim=True) / den - (z_kn[:, :, :3] * sf).sum(1, keepdim=True) / den
    shift = torch.cat([c.expand(-1, N, -1), torch.zeros_like(z_gen[:, :, 3:])], dim=2)
    z = torch.where(em.bool(), z_kn + shift, z_gen)
    z = torch.cat([orc.remove_mean_with_mask(z[:, :, :3], nmf), z[:, :, 3:]], dim=2)
    return torch.where(has, z, torch.where(em.bool(), z_kn, z_gen))


def replace_parts_mag(z_gen, xh_known, nm, fx, fh, alpha_s, sigma_s, raw):
    """A [B,N,D] float64 of the module docstring."""
    dt = torch.float64
    B, N, D = z_gen.shape
    nmf = (nm.reshape(B, N, 1) != 0).to(dt)
    fxf, _, em = masks_of(nm, fx, fh, dt)
    zg = z_gen.to(dt).abs()
    kn = torch.where(em != 0, xh_known.to(dt), torch.zeros((), dtype=dt))
    t_kn = (torch.as_tensor(alpha_s, dtype=dt) * kn).abs() + (torch.as_tensor(sigma_s, dtype=dt) * torch.cat(raw, dim=2).to(dt)).abs()
    nfix = fxf.sum(1, keepdim=True)
    has = nfix > 0
    den = nfix.clamp(min=1.0)
    smag = (zg[:, :, :3] * fxf).sum(1, keepdim=True) / den + (t_kn[:, :, :3] * fxf).sum(1, keepdim=True) / den
    t = torch.where(em != 0, t_kn, zg)
    tx = t[:, :, :3] + smag * fxf
    cnt = nmf.sum(1, keepdim=True).clamp(min=1.0)
    ax = tx + (tx * nmf).sum(1, keepdim=True) / cnt * nmf
    return torch.cat([torch.where(has, ax, zg[:, :, :3]), t[:, :, 3:]], dim=2)


def decode_fix_parts_ref(x, h, x_known, h_known, nm, fx, fh):
    """Behind the final decode, data units: h = h_known on the known channels, x = x_known + (mean_Fx(x) - mean_Fx(x_known)) on Fx."""
    fxf, fhf, _ = masks_of(nm, fx, fh, x.dtype)
    nfix = fxf.sum(1, keepdim=True)
    den = torch.where(nfix > 0, nfix, torch.ones_like(nfix))
    c = (x * fxf).sum(1, keepdim=True) / den - (x_known * fxf).sum(1, keepdim=True) / den
    return torch.where(fxf.bool(), x_known + c, x), torch.where(fhf.bool(), h_known, h)


def inpaint_parts_path_ref(lib, fnet, gg, path, T, z, nm, fx, fh, xh_known, R, seed, ids, k_lo=0, k_hi=None, x0_frames=None):
    """`tests.restraint_frame_reference.inpaint_path_ref` (itself `tests.test_inpaint_cpu.inpaint_steps_ref` on a path, with every
    round's eps^ from `fnet.net` - guided as `fnet` is) with `replace_parts_ref` in the place of `replace_ref`.  Returns the list of
    states (fp32) behind every transition; `x0_frames` receives (z, eps^) of every transition's last round."""
    from tests import guidance_reference as gr
    nmf = nm.float()
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
            z = gr.ancestral_on_eps(getattr(fnet, "c", fnet), z, eps, s, t, philox_raw(lib, seed, ids, draw(0), N), g32).float()
            z = replace_parts_ref(z, xh_known, nmf, fx, fh, alpha_s, sigma_s, philox_raw(lib, seed, ids, draw(1), N))
            if j < R - 1:
                e = orc.combined_noise(*philox_raw(lib, seed, ids, draw(2), N), nmf)
                z = alpha_ts.view(-1, 1, 1) * z + sigma_ts.view(-1, 1, 1) * e
        states.append(z)
    return states


# ----------------------------------------------------------------------------- the inputs of the kernel test

class _Case:
    pass


def kernel_case(N, F):
    """B = 7 molecules at D = 3 + F: nothing fixed; positions only on some nodes; all channels only on some nodes; the channels of
    CHANNELS (those below F) on nodes that overlap the position-fixed ones and on nodes that do not; everything fixed; a one-node
    molecule (position and channel 0); a partly masked molecule with mask bytes set and garbage known values on its masked rows.
    z_gen: N(0,1) on the valid rows with the x part mean-free, as the posterior step leaves it, 0 on the masked ones; the known
    positions sit around CENTRE / NV0 (normalised units)."""
    c = _Case()
    B, D = 7, 3 + F
    h = (N + 1) // 2
    c.B, c.N, c.F, c.D = B, N, F, D
    nm = torch.zeros(B, N, dtype=torch.bool)
    for b, n in enumerate((N, N, N, N, N, 1, h)):
        nm[b, :n] = True
    fx = torch.zeros(B, N, dtype=torch.bool)
    fh = torch.zeros(B, N, F, dtype=torch.bool)
    third = max(2, N // 3)
    fx[1, 1:1 + third] = True
    fh[2, N - third:] = True
    fx[3, :third] = True
    ch = [k for k in CHANNELS if k < F]
    for n in range(third - 1, min(N, 2 * third)):            # one node inside the position-fixed block, the rest outside it
        fh[3, n, ch] = True
    fx[4], fh[4] = True, True
    fx[5, 0], fh[5, 0, 0] = True, True
    fx[6, 0] = True
    fx[6, h - 1:] = True                                     # the last valid node and every masked row
    fh[6, 1] = True
    fh[6, h:, ::2] = True                                    # masked rows
    g = torch.Generator().manual_seed(1000 * N + F)
    z = torch.randn(B, N, D, generator=g) * nm[:, :, None]
    z = torch.cat([orc.remove_mean_with_mask(z[:, :, :3], nm[:, :, None].float()), z[:, :, 3:]], dim=2)
    z = torch.where(nm[:, :, None], z, torch.zeros(()))       # +0.0 on the masked rows (randn * False may be -0.0)
    known = torch.randn(B, N, D, generator=g)
    known[:, :, :3] = (torch.tensor(CENTRE) + 1.5 * torch.randn(B, N, 3, generator=g)) / NV0
    known[~nm] = 1.0e6 * torch.randn(int((~nm).sum()), D, generator=g)       # garbage on the masked rows
    c.nm, c.fx, c.fh, c.z, c.known = nm, fx, fh, z.contiguous(), known.contiguous()
    c.alpha, c.sigma = float(np.float32(0.8)), float(np.float32(0.6))
    c.seed, c.base, c.draw = 2022, 40, 1234
    return c


KERNEL_SHAPES = [(5, 1), (5, 8), (33, 1), (33, 8)]           # 33 * 11 > 256 elements: the second trip of the strided loop


def kernel_ratio(got, ref, mag):
    """Worst |got - ref| / (BOUND 2^-23 A); an element with A = 0 must be exact."""
    got, ref, mag = (np.asarray(v, dtype=np.float64) for v in (got, ref, mag))
    err = np.abs(got - ref)
    assert (err[mag == 0] == 0).all()
    return float((err / np.maximum(sref.BOUND * sref.U * mag, 1e-300)).max())
