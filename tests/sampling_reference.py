"""Float64 restatement of the sampler's three small kernels - `k_noise`, `k_post_step` (form 0) and `k_final_decode`
(hierdiff_amd/csrc/k_sampling.hpp; hd_noise, hd_posterior_step, hd_final_decode) - written from the formulas of the reference
(diffusion_qm9.py:445-456, :326-345, :302-310 + :174-179), numpy only: no torch and nothing imported from the product.  The
functions take the arrays the C entry points take (node mask bytes [B, N], coefficient rows rounded to float32, raw normals with one
row or B rows) and return the float64 value together with a MAGNITUDE array `A`: the same formula with every term replaced by its
absolute value and every mean by the mean of the absolute values over the molecule's counted nodes.  A correct float32 evaluation
stays within `BOUND * U * A` element by element:

    every term of an element passes at most 4 float32 roundings (divide or reciprocal, product, difference, sum); a molecule
    reduction in these kernels is at most 2 sequential adds per thread, a 6-step shuffle tree and 3 adds across wavefronts, under 12
    roundings against the sum of absolute values for mol * D <= 3300.  (4 + 12) * 2^-24 = 8 * 2^-23.

`cases()` are the fixed shapes of the tests (CPU and GPU tier see the same data), `kernel_f32` a plain float32 numpy evaluation of
the same formulas with a `mutant=` switch: the wrong kernels the bound has to reject (tests/test_sampling_reference_cpu.py)."""
import numpy as np

U = 2.0 ** -23
BOUND = 8.0

MUTANTS = ("count_is_mol", "no_final_recentre", "ceps_without_alpha", "coef_row_0_for_all", "noise_row_0_for_all", "noise_unmasked",
           "decode_centres_eps", "decode_h_unmasked", "index_with_D_11")


# ----------------------------------------------------------------------------- coefficient rows (float64, rounded once)

def _softplus(g):
    return np.logaddexp(0.0, g)


def _sigmoid(g):
    return np.exp(-_softplus(-g))


def step_coef_rows(gamma_s, gamma_t):
    """[rows, 4] float32 = {alpha_t|s, sigma2_t|s, sigma_t, sigma_t|s sigma_s / sigma_t}: hierdiff_amd.noise_model.step_coefficients
    (diffusion_qm9.py:181-204, :317-334) in float64, rounded once."""
    gs, gt = np.asarray(gamma_s, np.float64).reshape(-1), np.asarray(gamma_t, np.float64).reshape(-1)
    sigma2_ts = -np.expm1(_softplus(gs) - _softplus(gt))
    alpha_ts = np.exp(0.5 * (-_softplus(gt) + _softplus(gs)))            # logsigmoid(-g) = -softplus(g)
    sigma_s, sigma_t = np.sqrt(_sigmoid(gs)), np.sqrt(_sigmoid(gt))
    sigma = np.sqrt(sigma2_ts) * sigma_s / sigma_t
    return np.stack([alpha_ts, sigma2_ts, sigma_t, sigma], axis=1).astype(np.float32)


def decode_coef3(gamma_0):
    """float32 {sigma_0, alpha_0, sigma_x = exp(gamma_0 / 2)} of sample_p_xh_given_z0 (diffusion_qm9.py:294-301)."""
    g = float(gamma_0)
    return np.array([np.sqrt(_sigmoid(g)), np.sqrt(_sigmoid(-g)), np.exp(0.5 * g)], dtype=np.float32)


# ----------------------------------------------------------------------------- the float64 restatement

def _f64(a):
    return np.asarray(a, dtype=np.float64)


def _mask(nm):
    return (np.asarray(nm) != 0).astype(np.float64)[:, :, None]          # [B, n, 1]


def _rows(a, B):
    """One row broadcast over the batch (fix_noise / one coefficient row), or B rows."""
    a = _f64(a)
    assert a.shape[0] in (1, B)
    return np.broadcast_to(a, (B,) + a.shape[1:]) if a.shape[0] == 1 else a


def noise_ref(raw_x, raw_h, nm):
    """sample_combined_position_feature_noise: z = raw * m, x part minus (sum over nodes / count) * m.  raw_x [rows, n, 3], raw_h
    [rows, n, F], nm [B, n].  Returns (z, A) [B, n, 3 + F]."""
    m = _mask(nm)
    B = m.shape[0]
    cnt = m.sum(1, keepdims=True)
    zx, zh = _rows(raw_x, B) * m, _rows(raw_h, B) * m
    ax = np.abs(zx) + m * (np.abs(zx).sum(1, keepdims=True) / cnt)
    zx = zx - (zx.sum(1, keepdims=True) / cnt) * m
    return np.concatenate([zx, zh], axis=2), np.concatenate([ax, np.abs(zh)], axis=2)


def posterior_step_ref(zt, eps, coef, raw_x, raw_h, nm, mol):
    """sample_p_zs_given_zt after the network call (diffusion_qm9.py:326-345) on the first `mol` nodes: zt, eps [B, N, D], coef
    [rows, 4], raw_x [rows, mol, 3], raw_h [rows, mol, F], nm [B, N].  Returns (zs, A) [B, mol, D]."""
    zt, eps = _f64(zt)[:, :mol], _f64(eps)[:, :mol].copy()
    nm = np.asarray(nm)[:, :mol]
    m = _mask(nm)
    B = m.shape[0]
    cnt = m.sum(1, keepdims=True)
    cf = _rows(coef, B)
    alpha_ts, sigma2_ts, sigma_t, sigma = (cf[:, k].reshape(B, 1, 1) for k in range(4))
    c_eps = sigma2_ts / alpha_ts / sigma_t
    a_eps = np.abs(eps)
    a_eps[:, :, :3] += m * (a_eps[:, :, :3].sum(1, keepdims=True) / cnt)
    eps[:, :, :3] -= (eps[:, :, :3].sum(1, keepdims=True) / cnt) * m
    noise, a_noise = noise_ref(raw_x, raw_h, nm)
    zs = (zt / alpha_ts - c_eps * eps) + sigma * noise
    A = np.abs(zt / alpha_ts) + np.abs(c_eps) * a_eps + np.abs(sigma) * a_noise
    A[:, :, :3] += m * (A[:, :, :3].sum(1, keepdims=True) / cnt)
    zs[:, :, :3] -= (zs[:, :, :3].sum(1, keepdims=True) / cnt) * m
    return zs, A


def final_decode_ref(z0, eps, coef3, raw_x, raw_h, nm):
    """sample_p_xh_given_z0 after the network call + unnormalize with unit norm values: x = (z0 - sigma_0 eps) / alpha_0 +
    sigma_x noise on the x part (neither eps nor the result is centred), h = z0[..., 3:] * m.  Returns (x, h, A_x)."""
    z0, eps = _f64(z0), _f64(eps)
    m = _mask(nm)
    sigma_0, alpha_0, sigma_x = (float(v) for v in np.asarray(coef3, np.float32))
    noise, a_noise = noise_ref(raw_x, raw_h, nm)
    x = (z0[:, :, :3] - sigma_0 * eps[:, :, :3]) / alpha_0 + sigma_x * noise[:, :, :3]
    A = np.abs(z0[:, :, :3] / alpha_0) + np.abs(sigma_0 / alpha_0) * np.abs(eps[:, :, :3]) + abs(sigma_x) * a_noise[:, :, :3]
    return x, z0[:, :, 3:] * m, A


def ratio(got, ref, A, nm):
    """(worst |err| / (U * A) over the valid elements, number of masked elements that are not exactly 0)."""
    valid = np.broadcast_to(np.asarray(nm)[:, :ref.shape[1], None] != 0, ref.shape)
    err = np.abs(_f64(got) - ref)
    assert np.all(A[valid] > 0)
    return float(np.max(err[valid] / (U * A[valid]))), int(np.count_nonzero(_f64(got)[~valid]))


# ----------------------------------------------------------------------------- the cases

def _make_case(idx, name, N, valid, F, mol=None, coef_rows=None, noise_rows=None, offset=(3.0, -2.0, 1.0)):
    rng = np.random.Generator(np.random.PCG64([20261018, idx]))
    B, D = len(valid), 3 + F
    mol = N if mol is None else mol
    nm = np.zeros((B, N), dtype=np.uint8)
    for b, v in enumerate(valid):
        nm[b, (np.arange(v) if isinstance(v, int) else np.asarray(sorted(v)))] = 1
    assert nm[:, :mol].sum(1).min() >= 1                                 # an all-masked molecule is 0 / 0, as in the reference
    m = nm.astype(np.float32)[:, :, None]
    off = np.asarray(offset, dtype=np.float32).reshape(1, 1, 3) * m

    def state(shift):
        z = rng.standard_normal((B, N, D)).astype(np.float32) * m
        if shift:
            z[:, :, :3] += off
        return z
    zt, z0, eps = state(True), state(True), state(False)
    cr = B if coef_rows is None else coef_rows
    nr = B if noise_rows is None else noise_rows
    gamma_t = rng.uniform(-6.0, 8.0, size=cr)
    gamma_s = gamma_t - rng.uniform(0.001, 0.5, size=cr)
    c = dict(name=name, B=B, N=N, F=F, D=D, mol=mol, nm=nm, zt=zt, z0=z0, eps=eps, coef_rows=cr, noise_rows=nr,
             coef=step_coef_rows(gamma_s, gamma_t), coef3=decode_coef3(rng.uniform(-8.0, -4.0)),
             raw_x=rng.standard_normal((nr, mol, 3)).astype(np.float32), raw_h=rng.standard_normal((nr, mol, F)).astype(np.float32))
    # features of z0 that are NOT zero at masked nodes: outside the sampler's contract, the only input on which the `* m` of the
    # decode's h output does anything
    junk = rng.standard_normal((B, N, F)).astype(np.float32)
    c["z0_dirty"] = z0.copy()
    c["z0_dirty"][:, :, 3:] += junk * (1.0 - m)
    return c


_CASES = None


def cases():
    """name -> dict(B, N, F, D, mol, nm [B, N] uint8, zt, z0, eps [B, N, D] float32 (N(0,1) times the mask; the x part of zt and z0
    carries a per-molecule offset at the valid nodes), coef [coef_rows, 4], coef3 [3], raw_x [noise_rows, mol, 3], raw_h
    [noise_rows, mol, F], z0_dirty).  Built once; callers must not write into the arrays."""
    global _CASES
    if _CASES is None:
        pocket = [list(range(40)) + list(range(40, 64)), list(range(33)) + list(range(40, 64))]
        made = [
            _make_case(1, "S1", 8, [8, 5, 7, 3, 6, 1], 8),               # B = 6: partial last workgroup of the 4-per-workgroup kernels
            _make_case(2, "S2", 30, [30, 24, 1, 17], 8),                 # 330 elements: ragged second trip of e += 256
            _make_case(3, "S3", 70, [70, 65, 64, 2], 8, noise_rows=1),   # second trip of nn += 64; fix_noise broadcast
            _make_case(4, "S4", 300, [300, 257, 129], 8, offset=(30.0, -20.0, 10.0)),   # 13 trips, large offset
            _make_case(5, "S5", 64, pocket, 8, mol=40, coef_rows=1),     # mol_shape < N: stride mol out, N in; count over the molecule
            _make_case(6, "S6", 9, [9, 4, 1], 1),                        # D = 4
            _make_case(7, "S7", 25, [25, 24, 13], 12),                   # D = 15, 375 elements
            _make_case(8, "S8", 12, [{0, 2, 3, 7}, set(range(1, 12)), {5}], 8),          # masks that are not prefixes
        ]
        for c in made:
            for v in c.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
        _CASES = {c["name"]: c for c in made}
    return _CASES


STEP_CASES = ("S1", "S2", "S3", "S4", "S5", "S6", "S7", "S8")
FULL_CASES = ("S1", "S2", "S3", "S4", "S6", "S7", "S8")                  # hd_noise / hd_final_decode have no mol argument


# ----------------------------------------------------------------------------- float32 evaluation, with mutants

f32 = np.float32


def _reindex(a, width):
    """a[r, n, c] read at flat position n * width + c of its row block instead of n * d + c (wrapped into the block)."""
    R, n, d = a.shape
    idx = (np.arange(n)[:, None] * width + np.arange(d)[None, :]) % (n * d)
    return a.reshape(R, n * d)[:, idx]


def _noise_f32(raw_x, raw_h, nm, mutant):
    m = (np.asarray(nm) != 0).astype(f32)[:, :, None]
    B, n = m.shape[:2]
    rx, rh = np.asarray(raw_x, f32), np.asarray(raw_h, f32)
    if mutant == "index_with_D_11":
        rh = _reindex(rh, 8)
    if mutant == "noise_row_0_for_all":
        rx, rh = rx[:1], rh[:1]
    rx, rh = np.broadcast_to(rx, (B, n, 3)), np.broadcast_to(rh, (B, n, rh.shape[2]))
    cnt = f32(n) if mutant == "count_is_mol" else m.sum(1, keepdims=True, dtype=f32)
    if mutant == "noise_unmasked":
        zx, zh = rx.copy(), rh.copy()
    else:
        zx, zh = rx * m, rh * m
    zx = zx - (zx.sum(1, keepdims=True, dtype=f32) / cnt) * m
    return np.concatenate([zx, zh], axis=2).astype(f32)


def kernel_f32(entry, c, mutant=None, z0=None):
    """Float32 numpy evaluation of entry "noise" | "step" | "decode" on the case dict `c` (what a correct kernel computes, up to the
    order of its sums), or with `mutant` one of MUTANTS a wrong one.  Returns z | zs | (x, h)."""
    assert mutant is None or mutant in MUTANTS
    nm = c["nm"]
    if entry == "noise":
        return _noise_f32(c["raw_x"], c["raw_h"], nm, mutant)
    if entry == "decode":
        z0 = np.asarray(c["z0"] if z0 is None else z0, f32)
        eps = np.asarray(c["eps"], f32)
        if mutant == "index_with_D_11":
            z0, eps = _reindex(z0, 11), _reindex(eps, 11)
        m = (nm != 0).astype(f32)[:, :, None]
        sigma_0, alpha_0, sigma_x = (f32(v) for v in c["coef3"])
        ex = eps[:, :, :3]
        if mutant == "decode_centres_eps":
            ex = ex - (ex.sum(1, keepdims=True, dtype=f32) / m.sum(1, keepdims=True, dtype=f32)) * m
        noise = _noise_f32(c["raw_x"], c["raw_h"], nm, mutant)
        x = (f32(1.0) / alpha_0) * (z0[:, :, :3] - sigma_0 * ex) + sigma_x * noise[:, :, :3]
        h = z0[:, :, 3:] if mutant == "decode_h_unmasked" else z0[:, :, 3:] * m
        return x.astype(f32), h.astype(f32)
    assert entry == "step"
    mol = c["mol"]
    zt, eps = np.asarray(c["zt"], f32), np.asarray(c["eps"], f32)
    if mutant == "index_with_D_11":
        zt, eps = _reindex(zt, 11), _reindex(eps, 11)
    zt, eps = zt[:, :mol], eps[:, :mol].copy()
    nmm = nm[:, :mol]
    m = (nmm != 0).astype(f32)[:, :, None]
    B = m.shape[0]
    cnt = f32(mol) if mutant == "count_is_mol" else m.sum(1, keepdims=True, dtype=f32)
    cf = np.asarray(c["coef"], f32)
    if mutant == "coef_row_0_for_all":
        cf = cf[:1]
    cf = np.broadcast_to(cf, (B, 4))
    alpha_ts, sigma2_ts, sigma_t, sigma = (cf[:, k].reshape(B, 1, 1) for k in range(4))
    c_eps = sigma2_ts / sigma_t if mutant == "ceps_without_alpha" else (sigma2_ts / alpha_ts) / sigma_t
    eps[:, :, :3] -= (eps[:, :, :3].sum(1, keepdims=True, dtype=f32) / cnt) * m
    noise = _noise_f32(c["raw_x"], c["raw_h"], nmm, mutant)
    zs = ((zt / alpha_ts - c_eps * eps) + sigma * noise).astype(f32)
    if mutant != "no_final_recentre":
        zs[:, :, :3] -= (zs[:, :, :3].sum(1, keepdims=True, dtype=f32) / cnt) * m
    return zs
