"""CPU restatement of classifier-free guidance (hd_guide_combine / hd_sample_path_guided; algorithm in include/hierdiff_hip.h,
"Classifier-free guidance"), the yardstick of tests/test_guidance_cpu.py and tests/test_gpu_guidance.py.

Built from `oracle.egnn_oracle` alone, through the pieces tests/edit_reference.py already wraps (`RefNet`: dynamics_forward /
posterior_step / final_decode): the network runs under both contexts, `combine_ref` forms eps_u + w (eps_c - eps_u) (and the
rescale), and the transition is restated on that given eps:
  eta = 1   the oracle's `posterior_step` arithmetic line for line (same operations in the same order on the same dtypes, so with
            every w_b = 1 the chain is `partial_chain_ref`'s bit for bit);
  eta < 1   `down_row` in Python floats, float64 arithmetic, as `partial_chain_ref` does.
The state is kept in the network's dtype (fp32: rounded once per transition, as the device loop keeps it); `RefNet(dtype=float64)`
gives the double-precision form of the same chain."""
import numpy as np
import torch

from oracle import egnn_oracle as orc
from tests.edit_reference import RefNet, _centre_x, down_row


def combine_ref(eps_c, eps_u, w, phi, node_mask, dtype=torch.float64):
    """out [B,N,D] in `dtype`: per molecule w_b == 1 -> eps_c, w_b == 0 -> eps_u (phi ignored); otherwise g = eps_u + w_b (eps_c -
    eps_u) and, with phi > 0, f g with f = phi sqrt(S_c / S_g) + (1 - phi), S_* the sums of squared deviations from the mean over the
    molecule's valid entries (all D columns); S_g == 0 or a non-finite quotient: f = 1.  Masked entries 0.  float32: the kernel's
    arithmetic (one subtraction, one multiply-add - not fused here: a difference of one rounding), the factor from float64 sums."""
    ec, eu = eps_c.to(dtype), eps_u.to(dtype)
    B, N, D = ec.shape
    m = node_mask.reshape(B, N, 1).to(dtype)
    wv = torch.as_tensor(w, dtype=torch.float32).reshape(-1)
    wv = wv.expand(B) if wv.numel() == 1 else wv
    out = torch.zeros_like(ec)
    for b in range(B):
        wb = float(wv[b])
        if wb == 1.0:
            out[b] = ec[b] * m[b]
            continue
        if wb == 0.0:
            out[b] = eu[b] * m[b]
            continue
        g = (eu[b] + torch.tensor(wb, dtype=dtype) * (ec[b] - eu[b])) * m[b]
        if phi > 0.0:
            valid = m[b].expand(N, D).bool()
            c64, g64 = ec[b].double()[valid], g.double()[valid]
            r = 1.0
            if c64.numel() > 0:
                s_c, s_g = float(((c64 - c64.mean()) ** 2).sum()), float(((g64 - g64.mean()) ** 2).sum())
                if s_g > 0.0 and np.isfinite(np.sqrt(s_c / s_g)):
                    r = float(np.sqrt(s_c / s_g))
            g = torch.tensor(phi * r + (1.0 - phi), dtype=dtype) * g
        out[b] = g
    return out


class GuidedNet:
    """eps^ of a guided network call: `net_c` / `net_u` are two `RefNet`s on the same weights and masks under the context and the
    null context."""

    def __init__(self, net_c: RefNet, net_u: RefNet, w, phi):
        assert net_c.dtype == net_u.dtype
        self.c, self.u, self.w, self.phi, self.dtype = net_c, net_u, w, float(phi), net_c.dtype
        self.nm = net_c.nm

    def net(self, z, t_idx):
        return combine_ref(self.c.net(z, t_idx), self.u.net(z, t_idx), self.w, self.phi, self.nm, dtype=self.dtype)


def ancestral_on_eps(net: RefNet, z, eps, s, t, raw, gg):
    """`oracle.egnn_oracle.posterior_step` (mol_shape = N) behind its network call, on a given eps, operation for operation."""
    with net, torch.no_grad():
        B = z.shape[0]
        nm = orc._t(net.nm)
        gamma_s, gamma_t = orc._t(gg[s].expand(B, 1)).view(-1, 1), orc._t(gg[t].expand(B, 1)).view(-1, 1)
        sigma2_ts, sigma_ts, alpha_ts = orc.sigma_and_alpha_t_given_s(gamma_t, gamma_s)
        sigma2_ts, sigma_ts, alpha_ts = (v.view(-1, 1, 1) for v in (sigma2_ts, sigma_ts, alpha_ts))
        sigma_s = torch.sqrt(torch.sigmoid(gamma_s)).view(-1, 1, 1)
        sigma_t = torch.sqrt(torch.sigmoid(gamma_t)).view(-1, 1, 1)
        zt = orc._t(z)
        eps = orc._t(eps).clone()
        eps[:, :, :3] = orc.remove_mean_with_mask(eps[:, :, :3], nm)
        mu = zt / alpha_ts - (sigma2_ts / alpha_ts / sigma_t) * eps
        sigma = sigma_ts * sigma_s / sigma_t
        noise = orc.combined_noise(orc._t(raw[0]), orc._t(raw[1]), nm)
        zs = mu + sigma * noise
        return torch.cat([orc.remove_mean_with_mask(zs[:, :, :3], nm), zs[:, :, 3:]], dim=2)


def decode_on_eps(net: RefNet, z0, eps, raw, gg):
    """`oracle.egnn_oracle.final_decode` (unit normalisation) behind its network call, on a given eps."""
    with net, torch.no_grad():
        B = z0.shape[0]
        z0, nm = orc._t(z0), orc._t(net.nm)
        gamma_0 = orc._t(gg[0].expand(B, 1)).view(-1, 1)
        sigma_x = torch.exp(-(-0.5 * gamma_0)).unsqueeze(1)
        sigma_0 = torch.sqrt(torch.sigmoid(gamma_0)).view(-1, 1, 1)
        alpha_0 = torch.sqrt(torch.sigmoid(-gamma_0)).view(-1, 1, 1)
        mu_x = 1.0 / alpha_0 * (z0 - sigma_0 * orc._t(eps))
        xh = mu_x + sigma_x * orc.combined_noise(orc._t(raw[0]), orc._t(raw[1]), nm)
        return xh[:, :, :3] * 1.0, (z0[:, :, 3:] * 1.0 + 0.0) * nm


def guided_chain_ref(gnet: GuidedNet, gg, path, eta, z, node_mask, raws, decode=True):
    """The guided reverse chain on the descending `path` from the state z at path[0], with injected normals raws = [one pair per
    transition (, the decode)].  Returns (x, h, z_0), or z_0 alone with decode=False."""
    dt = gnet.dtype
    nmf = node_mask.to(dt)
    nmd = node_mask.to(torch.float64)
    z = z.to(dt)
    for k, (t, s) in enumerate(zip(path[:-1], path[1:])):
        eps = gnet.net(z, t)
        if eta == 1.0:
            z = ancestral_on_eps(gnet.c, z, eps, s, t, raws[k], gg).to(dt)
            continue
        a, b, c = down_row(float(gg[s]), float(gg[t]), eta)
        eps = _centre_x(eps.double(), nmd)
        zs = a * z.double() - b * eps
        if c != 0.0:
            zs = zs + c * orc.combined_noise(raws[k][0], raws[k][1], nmf).double()
        z = _centre_x(zs, nmd).to(dt)
    if not decode:
        return z
    x, h = decode_on_eps(gnet.c, z, gnet.net(z, 0), raws[len(path) - 1], gg)
    return x.to(dt), h.to(dt), z


# ----------------------------------------------------------------------------- the shared parity cases
# (name, molecules, path builder arguments, eta, w, phi).  w: a scalar, or per molecule (cut to the batch).  The bar of every case is
# tests/test_gpu_fewstep.py's BAR (rel-L2 1e-3 on the final x and h), the one the unguided chain of the same (T, K, eta) is held to.
BAR = 1e-3
W_ROWS = [2.5, 1.0, 0.3, -0.5, 1.7]
PARITY = []
for _n, _mols in (("main", [7, 4, 1]), ("wrap", [30, 17])):
    for _pname, _few in (("identity", dict(eta=1.0)), ("K7eta0", dict(steps=7, eta=0.0)), ("K5eta05", dict(steps=5, eta=0.5))):
        for _wname, _w in (("w2.5", 2.5), ("wrows", W_ROWS)):
            for _phi in (0.0, 0.7):
                PARITY.append((f"{_n}-{_pname}-{_wname}-phi{_phi}", _mols, _few, _w, _phi))


def scale_for(w, B):
    return w if not isinstance(w, list) else torch.tensor(w[:B], dtype=torch.float32)


def null_ctx(nm, value=0.0):
    return torch.full(tuple(nm.shape[:2]) + (1,), float(value)) * nm.float()
