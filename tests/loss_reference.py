"""A plain-torch restatement of the training loss behind the network call, and the designed inputs its kernel is tested on.

`vlb_loss_ref` / `vlb_zt_ref` restate what `hd_vlb_loss_forward` / `hd_vlb_zt` (csrc/k_loss.hpp) compute, written from the oracle's
`nll_forward` (oracle/egnn_oracle.py, training mode: one network call, the t == 0 rows switched to the L0 term) - not from the
kernel.  They run in the dtype of their inputs and are differentiated by autograd only: float64 is the reference of
tests/test_gpu_loss_kernels.py, float32 is "the reference's own arithmetic" whose distance from float64 is printed next to the
kernel's.  tests/test_loss_reference_cpu.py pins the restatement to numbers the reference produced (fixtures F9 / F12 / F13 / F20)
and checks that every designed input is well conditioned: the fp32 restatement itself meets the bars the kernel is held to.

The designed inputs (`vlb_inputs`) put the integer-feature likelihood  log(Phi((c + 1/2) / s0) - Phi((c - 1/2) / s0) + 1e-10)  where
it matters.  Every masked-in integer element of a t = 0 molecule lies in one of two zones:
  A  the float64 bracket is >= 1e-3: |c| up to ~3 s0, or c within a few s0 of +-1/2 (one of the two cdf arguments of order 1);
  C  both cdf arguments beyond 8 on the same side: the bracket is exactly 0 in fp32 and < 1e-15 in float64, the result log(1e-10).
The band in between (1e-10 < bracket < 1e-3) is left out on purpose: there the reference's fp32 `Phi - Phi` is quantised at 6e-8
and is itself far from float64 - a property of the reference's expression, which the kernel keeps, not of the kernel.
"""
import functools
import math

import numpy as np
import torch

N_DIMS = 3
T_STEPS = 1000.0
LOG2_F32 = float(np.float32(math.log(2.0)))

# bars (tests/test_gpu_training.py GRAD_TOL; the value tier of tests/fuzz_egcl_grads.py)
GRAD_TOL = 1e-4
VALUE_TOL = 1e-5


# ----------------------------------------------------------------------------- the restatement

def vlb_zt_ref(xh, eps, gt):
    """z_t = alpha(g_t) xh + sigma(g_t) eps, alpha = sqrt(sigmoid(-g)), sigma = sqrt(sigmoid(g)).  gt [B] (one value per molecule) or
    any shape that broadcasts from the left, up to one value per element."""
    g = gt.reshape(tuple(gt.shape) + (1,) * (xh.dim() - gt.dim()))
    return torch.sqrt(torch.sigmoid(-g)) * xh + torch.sqrt(torch.sigmoid(g)) * eps


def _std_normal_cdf(v):
    return 0.5 * (1.0 + torch.erf(v / math.sqrt(2.0)))


def _sum_rows(v):
    return v.reshape(v.shape[0], -1).sum(dim=-1)


def int_likelihood_args(h_int, z_int, g, nv2, nb2):
    """The two cdf arguments of the integer-feature likelihood: ((c + 1/2) / s0, (c - 1/2) / s0) with
    c = round(h nv2 + nb2) - (z nv2 + nb2) (torch.round: half to even), s0 = sigma(g) nv2."""
    sigma_0 = torch.sqrt(torch.sigmoid(g)) * nv2
    centred = torch.round(h_int * nv2 + nb2) - (z_int * nv2 + nb2)
    return (centred + 0.5) / sigma_0, (centred - 0.5) / sigma_0


def vlb_terms(net, zt, xh, eps, nm, gam4, t_int, *, int_nf, cont_nf, l2_train, T, nv2, nb2, log_nv0, gt_int=None):
    """The pieces of the loss per molecule: K (KL to the prior), L0 (t = 0 term), Lpos (t > 0 term), C0 (log constants), delta (volume
    term), est (estimator weight), is0, err.  gt_int [B, N, int_nf]: g_t per integer element instead of gam4[1] per molecule (used
    only to split d loss / d g_t into its per-element terms for the scale of a bar)."""
    B, N, D = xh.shape
    nd, F_in = N_DIMS, D - N_DIMS
    m = nm.reshape(B, N, 1)
    gamma_s, gamma_t, gamma_0, gamma_T = gam4[0], gam4[1], gam4[2], gam4[3]

    def err_of(e, o):
        v = _sum_rows((e - o) ** 2)
        return v / ((nd + F_in) * o.shape[1]) if l2_train else v

    error = err_of(eps, net)
    snr_weight = torch.ones_like(error) if l2_train else torch.exp(-(gamma_s - gamma_t)) - 1.0
    loss_t_pos = 0.5 * snr_weight * error

    n_nodes = nm.sum(1)
    log_sigma = 0.5 * gamma_0
    const = -0.5 * math.log(2.0 * math.pi)
    neg_log_constants = -((n_nodes - 1) * nd * (-log_sigma + const)) - (n_nodes * F_in * (-log_sigma + const))
    if l2_train:
        neg_log_constants = torch.zeros_like(neg_log_constants)

    # KL(q(z_T | x) || N(0, 1)): h masked, x on the (n - 1) * 3 dimensional subspace and NOT masked
    mu = torch.sqrt(torch.sigmoid(-gamma_T)).view(B, 1, 1) * xh
    sig_T = torch.sqrt(torch.sigmoid(gamma_T))
    s3 = sig_T.view(B, 1, 1)
    kl_h = _sum_rows((torch.log(1.0 / s3) + 0.5 * (s3 ** 2 + mu[:, :, nd:] ** 2) - 0.5) * m)
    d = (n_nodes - 1) * nd
    kl_x = d * torch.log(1.0 / sig_T) + 0.5 * (d * sig_T ** 2 + _sum_rows(mu[:, :, :nd] ** 2)) - 0.5 * d
    kl_prior = kl_x + kl_h

    # -log p(x, h | z_0) without constants, evaluated at z_t with g_t (training mode)
    err_x = err_of(eps[:, :, :nd], net[:, :, :nd])
    # the continuous noise columns against a STRIDED slice of the prediction: `: nd + int_nf : nd + int_nf + cont_nf` is column 0
    err_c = err_of(eps[:, :, nd + int_nf:nd + int_nf + cont_nf], net[:, :, :nd + int_nf:nd + int_nf + cont_nf])
    g_int = gamma_t.view(B, 1, 1) if gt_int is None else gt_int
    ap, am = int_likelihood_args(xh[:, :, nd:nd + int_nf], zt[:, :, nd:nd + int_nf], g_int, nv2, nb2)
    log_int = torch.log(_std_normal_cdf(ap) - _std_normal_cdf(am) + 1e-10)
    loss_0 = 0.5 * err_x + 0.5 * err_c - _sum_rows(log_int * m)

    is0 = (t_int == 0).to(xh.dtype)
    est = 1.0 if l2_train else T + 1.0
    delta = torch.zeros_like(d) if l2_train else -d * log_nv0
    return dict(K=kl_prior, L0=loss_0, Lpos=loss_t_pos, C0=neg_log_constants, delta=delta, est=est, is0=is0, err=error)


def vlb_loss_ref(net, zt, xh, eps, nm, gam4, t_int, *, int_nf, cont_nf, l2_train, T, nv2, nb2, log_nv0):
    """(loss [B], err [B]) of compute_loss in training mode behind the network call.  net / zt / xh / eps [B, N, D], nm [B, N],
    gam4 [4, B] = gamma at (s, t, 0, 1), t_int [B]; masked-out nodes of net / eps / xh are zero."""
    p = vlb_terms(net, zt, xh, eps, nm, gam4, t_int, int_nf=int_nf, cont_nf=cont_nf, l2_train=l2_train, T=T, nv2=nv2, nb2=nb2,
                  log_nv0=log_nv0)
    loss_t = p["L0"] * p["is0"] + (1.0 - p["is0"]) * p["Lpos"]
    return p["K"] + p["est"] * loss_t + p["C0"] - p["delta"], p["err"]


# ----------------------------------------------------------------------------- designed inputs

# (B, N, D, int_nf, cont_nf): N D = 253 / 264 around one trip of the 256-thread loops, 330 the headline training shape, 288 'elem'
# features, 1067 five trips with a ragged last one, 11 a single node, 360 a spare column behind the features
VLB_SHAPES = [(5, 23, 11, 5, 3), (5, 24, 11, 5, 3), (7, 30, 11, 5, 3), (4, 48, 6, 3, 0), (3, 97, 11, 5, 3), (2, 1, 11, 5, 3),
              (2, 30, 12, 5, 3)]
# (l2_train, nv2, nb2, log_nv0)
VLB_VARIANTS = [(l2, nv2, nb2, lg) for l2 in (0, 1) for nv2, nb2 in ((1.0, 0.0), (10.0, 0.5)) for lg in (0.0, LOG2_F32)]
MIN_GAMMA_STEP = 0.02           # g_t - g_s below this: the reference's fp32 exp(g_t - g_s) - 1 loses more than the value bar


def _t0_rows(B):
    """t = 0 rows interleaved with the others; the first and the last molecule are t = 0 rows."""
    return [b % 2 == 0 or b == B - 1 for b in range(B)]


@functools.lru_cache(maxsize=None)
def vlb_inputs(B, N, D, int_nf, cont_nf, nv2, nb2):
    """fp32 CPU tensors net, zt, xh, eps [B, N, D], nm [B, N], gam [4, B], t_int [B], gout [B] (shared by both tiers: do not write)."""
    rng = np.random.Generator(np.random.PCG64([B, N, D, int_nf, cont_nf, int(nv2), int(2 * nb2)]))
    nd = N_DIMS
    t0 = np.array(_t0_rows(B))
    # ragged molecules: the last one full, a t = 0 row of one node (molecule 2, or 0 in a small batch), a large t > 0 molecule
    sizes = rng.integers(min(2, N), N + 1, size=B)
    sizes[B - 1] = N
    sizes[2 if B >= 4 else 0] = 1
    if B >= 3:
        sizes[1] = max(1, N - 1 - int(rng.integers(0, max(1, N // 3))))
    nm = (np.arange(N)[None, :] < sizes[:, None]).astype(np.float64)
    m3 = nm[:, :, None]
    t_int = np.where(t0, 0.0, rng.integers(1, int(T_STEPS) + 1, size=B).astype(np.float64))
    if B >= 4:
        t_int[3] = T_STEPS if not t0[3] else t_int[3]

    # schedule values, rounded to fp32 first: both precisions see the same numbers
    g0 = rng.uniform(-8.0, -3.0, B)
    gT = rng.uniform(5.0, 12.0, B)
    gT[B // 2] = 16.0
    gt = np.where(t0, rng.uniform(-8.0, -3.0, B), rng.uniform(-5.0, 6.0, B))
    gt[0], gt[B - 1] = -3.25, -7.5
    step = np.where(t0, rng.uniform(0.1, 0.8, B), rng.uniform(0.05, 2.5, B))
    if B >= 3:
        step[1] = 0.0205                                     # just above MIN_GAMMA_STEP after rounding
    gt = gt.astype(np.float32).astype(np.float64)
    gs = (gt - step).astype(np.float32).astype(np.float64)
    gam = np.stack([gs, gt, g0, gT])

    k_int = rng.integers(0, 5, size=(B, N, int_nf)).astype(np.float64)
    xh = rng.standard_normal((B, N, D))
    xh[:, :, nd:nd + int_nf] = (k_int - nb2) / nv2 + rng.uniform(-0.2, 0.2, (B, N, int_nf)) / nv2
    xh = (xh * m3).astype(np.float32).astype(np.float64)
    eps = (rng.standard_normal((B, N, D)) * m3).astype(np.float32).astype(np.float64)
    # The prediction of the t > 0 rows lies far from the noise (|net| ~ 16).  The prior term K carries n F roundings of
    # log(1 / sigma_T) + sigma_T^2 / 2 - 1 / 2 - about 6e-8 each and all alike, where the true value (1 - sigma_T^2)^2 / 4 is far
    # smaller for every g_T >= 5 - so the reference's fp32 K is off by ~ n F 6e-8 in absolute terms.  The vlb loss hides that
    # behind its log constants and the (T + 1) weight; the `l2` loss of a t > 0 row is just K + E / (2 D N), and with E / (D N) ~ 1
    # the reference's own arithmetic would miss the 1e-5 bar from n F ~ 170 on.  (t = 0 rows: the likelihood term is large.)
    net = (rng.standard_normal((B, N, D)) * np.where(t0, 1.0, 16.0)[:, None, None] * m3).astype(np.float32)

    alpha, sigma = np.sqrt(1.0 / (1.0 + np.exp(gt))), np.sqrt(1.0 / (1.0 + np.exp(-gt)))
    zt = alpha[:, None, None] * xh + sigma[:, None, None] * eps
    # the integer columns of the t = 0 rows: c / s0 placed on purpose (z_t is a free input of the kernel)
    cdf = lambda v: 0.5 * (1.0 + np.vectorize(math.erf)(v / math.sqrt(2.0)))
    for b in np.nonzero(t0)[0]:
        s0 = sigma[b] * nv2
        shape = (N, int_nf)
        sign = rng.choice([-1.0, 1.0], shape)
        near0 = rng.uniform(-3.0, 3.0, shape) * s0                               # zone A: |c| up to 3 s0
        edge = sign * (0.5 + rng.uniform(-3.0, 2.5, shape) * s0)                 # zone A: one cdf argument of order 1
        c_a = np.where(rng.random(shape) < 0.5, near0, edge)
        for _ in range(60):                                                      # pull the few with a small bracket towards c = 0
            small = cdf((c_a + 0.5) / s0) - cdf((c_a - 0.5) / s0) < 3e-3
            if not small.any():
                break
            c_a = np.where(small, 0.8 * c_a, c_a)
        c_c = sign * (0.5 + rng.uniform(9.0, 12.0, shape) * s0)                  # zone C: both arguments beyond 8
        # masked-in elements alternate between the zones (both present from two elements on); masked-out nodes get zone A values,
        # so that a sum which forgets the mask is wrong
        order = (np.arange(N * int_nf).reshape(shape) + int(rng.integers(0, 2))) % 2 == 0
        c = np.where(order | (nm[b][:, None] == 0), c_a, c_c)
        hint = np.round(xh[b, :, nd:nd + int_nf] * nv2 + nb2)
        zt[b, :, nd:nd + int_nf] = (hint - c - nb2) / nv2
    gout = rng.standard_normal(B) * 0.3 + np.where(rng.random(B) < 0.5, 0.5, -0.5)
    gout[0], gout[B - 1] = 0.0, -abs(gout[B - 1]) - 0.1
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    return dict(net=f32(net), zt=f32(zt), xh=f32(xh), eps=f32(eps), nm=f32(nm), gam=f32(gam), t_int=f32(t_int), gout=f32(gout))


def vlb_consts(shape, variant):
    _, _, _, int_nf, cont_nf = shape
    l2, nv2, nb2, lg = variant
    return dict(int_nf=int_nf, cont_nf=cont_nf, l2_train=bool(l2), T=T_STEPS, nv2=nv2, nb2=nb2, log_nv0=lg)


def vlb_case_inputs(shape, variant):
    return vlb_inputs(*shape, variant[1], variant[2])


def int_zones(inp, consts):
    """float64 view of the integer elements that count (masked-in, t = 0 rows): (bracket, ap, am) as 1-D tensors, and the molecule
    index of each."""
    nd, k = N_DIMS, consts["int_nf"]
    xh, zt = inp["xh"].double(), inp["zt"].double()
    B, N, _ = xh.shape
    ap, am = int_likelihood_args(xh[:, :, nd:nd + k], zt[:, :, nd:nd + k], inp["gam"][1].double().view(B, 1, 1), consts["nv2"],
                                 consts["nb2"])
    sel = ((inp["nm"] > 0)[:, :, None] & (inp["t_int"] == 0)[:, None, None]).expand(B, N, k)
    mol = torch.arange(B).view(B, 1, 1).expand(B, N, k)[sel]
    return (_std_normal_cdf(ap) - _std_normal_cdf(am))[sel], ap[sel], am[sel], mol


@torch.enable_grad()
def vlb_evaluate(inp, consts, dtype):
    """The restatement and its autograd gradients of sum(loss * gout) in `dtype`; everything returned as float64."""
    c = {k: v.to(dtype) for k, v in inp.items()}
    net, zt, gam = (c[k].clone().requires_grad_(True) for k in ("net", "zt", "gam"))
    loss, err = vlb_loss_ref(net, zt, c["xh"], c["eps"], c["nm"], gam, c["t_int"], **consts)
    (loss * c["gout"]).sum().backward()
    return dict(loss=loss.detach().double(), err=err.detach().double(), dnet=net.grad.double(), dzt=zt.grad.double(),
                dgam=gam.grad.double())


@torch.enable_grad()
def vlb_scales(inp, consts):
    """The scales of the relative bars, all from the float64 restatement: loss [B] = |K| + est |L| + |C0| + |delta| (L the term
    the row's t selects), dgam [4, B] = the sum of the absolute values of the terms d(loss gout) / d gamma is made of (K, C0, the
    t > 0 term, and the t = 0 likelihood element by element - its terms have both signs)."""
    c = {k: v.double() for k, v in inp.items()}
    B, N, _ = c["xh"].shape
    gam = c["gam"].clone().requires_grad_(True)
    gt_int = c["gam"][1].view(B, 1, 1).expand(B, N, consts["int_nf"]).clone().requires_grad_(True)
    p = vlb_terms(c["net"], c["zt"], c["xh"], c["eps"], c["nm"], gam, c["t_int"], gt_int=gt_int, **consts)
    sel = p["L0"] * p["is0"] + (1.0 - p["is0"]) * p["Lpos"]
    loss_scale = (p["K"].abs() + p["est"] * sel.abs() + p["C0"].abs() + p["delta"].abs()).detach()
    dgam = torch.zeros(4, B, dtype=torch.float64)
    for term in (p["K"], p["C0"], p["est"] * (1.0 - p["is0"]) * p["Lpos"]):
        if term.requires_grad:
            g, = torch.autograd.grad((term * c["gout"]).sum(), gam, retain_graph=True, allow_unused=True)
            if g is not None:
                dgam += g.abs()
    g, = torch.autograd.grad((p["est"] * p["is0"] * p["L0"] * c["gout"]).sum(), gt_int, allow_unused=True)
    if g is not None:
        dgam[1] += g.abs().sum(dim=(1, 2))
    return loss_scale, dgam


def rel_l2_t(got, ref):
    n = float(ref.norm())
    d = float((got.double() - ref).norm())
    return d / n if n > 0 else (0.0 if d == 0 else math.inf)


def _scaled_worst(got, ref, scale, tol):
    """max |got - ref| / (tol * scale); an element whose scale is 0 must be exactly the reference's 0."""
    diff = (got.double() - ref).abs()
    if bool(((scale == 0) & (diff != 0)).any()):
        return math.inf
    ok = scale > 0
    return float((diff[ok] / (tol * scale[ok])).max()) if bool(ok.any()) else 0.0


def vlb_ratios(got, ref, scales):
    """Measured error over bar for every checked quantity (pass: each < 1).  got / ref: dicts as `vlb_evaluate` returns them."""
    loss_scale, dgam_scale = scales
    return dict(loss=_scaled_worst(got["loss"], ref["loss"], loss_scale, VALUE_TOL),
                err=_scaled_worst(got["err"], ref["err"], ref["err"].abs(), VALUE_TOL),
                dnet=rel_l2_t(got["dnet"], ref["dnet"]) / GRAD_TOL,
                dzt=rel_l2_t(got["dzt"], ref["dzt"]) / GRAD_TOL,
                dgam=_scaled_worst(got["dgam"], ref["dgam"], dgam_scale, GRAD_TOL))


@functools.lru_cache(maxsize=None)
def vlb_expected(shape, variant):
    """(float64 results, scales, ratios of the fp32 restatement on the CPU) of one case, computed once."""
    inp, consts = vlb_case_inputs(shape, variant), vlb_consts(shape, variant)
    ref = vlb_evaluate(inp, consts, torch.float64)
    scales = vlb_scales(inp, consts)
    return ref, scales, vlb_ratios(vlb_evaluate(inp, consts, torch.float32), ref, scales)


# ----------------------------------------------------------------------------- hd_vlb_zt

ZT_SIZES = [11, 253, 256, 257, 1067]
ZT_GAMMAS = [-30.0, -10.0, 0.0, 10.0, 30.0]


@functools.lru_cache(maxsize=None)
def zt_inputs(ND):
    rng = np.random.Generator(np.random.PCG64([77, ND]))
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    B = len(ZT_GAMMAS)
    return dict(xh=f32(rng.standard_normal((B, ND)) * 2.0), eps=f32(rng.standard_normal((B, ND))), gt=f32(np.array(ZT_GAMMAS)),
                dzt=f32(rng.standard_normal((B, ND))))


@torch.enable_grad()
def zt_evaluate(inp, dtype):
    """(z_t, d sum(z_t dzt) / d g_t, and - float64 only - the sum of the absolute per-element terms of that gradient)."""
    c = {k: v.to(dtype) for k, v in inp.items()}
    gt = c["gt"].clone().requires_grad_(True)
    zt = vlb_zt_ref(c["xh"], c["eps"], gt)
    (zt * c["dzt"]).sum().backward()
    g_el = c["gt"].view(-1, 1).expand_as(c["xh"]).clone().requires_grad_(True)
    (vlb_zt_ref(c["xh"], c["eps"], g_el) * c["dzt"]).sum().backward()
    return zt.detach().double(), gt.grad.double(), g_el.grad.double().abs().sum(1)


# ----------------------------------------------------------------------------- hd_linear

LINEAR_SHAPES = [(1, 1, 1), (7, 5, 3), (257, 8, 49), (300, 12, 1), (33, 256, 256), (1000, 49, 50)]


@functools.lru_cache(maxsize=None)
def linear_inputs(M, K, N):
    """x [M, K], W [N, K], b [N] in fp32 with pre-activations of standard deviation ~40: they span +-100, both activations deep in
    saturation on either side."""
    rng = np.random.Generator(np.random.PCG64([5, M, K, N]))
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    x, W, b = rng.standard_normal((M, K)), rng.standard_normal((N, K)) * 40.0 / math.sqrt(K), rng.standard_normal(N) * 10.0
    if M * N < 32:                                  # too few outputs to span anything by chance: +-100 by hand
        x[:] = 1.25
        W[:] = 80.0 / K * np.where(np.arange(N) % 2 == 0, 1.0, -1.0)[:, None]
        b *= 0.1
    return f32(x), f32(W), f32(b)


def linear_ref(x, W, b, act):
    """act(x W^T + b) in the dtype of the inputs; act 0 none, 1 SiLU, 2 sigmoid."""
    y = x @ W.t()
    if b is not None:
        y = y + b
    return y if act == 0 else (y * torch.sigmoid(y) if act == 1 else torch.sigmoid(y))
