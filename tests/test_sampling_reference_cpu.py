"""CPU tier of the sampling-kernel tests: the float64 restatement of tests/sampling_reference.py is the oracle's arithmetic
(`orc.combined_noise`, `orc.posterior_step`, `orc.final_decode`) at three feature widths; a plain float32 evaluation of it stays
inside the bound `BOUND * U * A` the GPU tier holds the kernels to (tests/test_gpu_sampling_kernels.py); and every wrong kernel on the
list - wrong count, no final re-centring, wrong coefficient, wrong row, unmasked noise, wrong width - leaves it."""
import numpy as np
import pytest
import torch

from hierdiff_amd.weights import synthetic_state_dict
from oracle import egnn_oracle as orc
from tests import sampling_reference as sr

CASES = sr.cases()


# ----------------------------------------------------------------------------- the restatement is the oracle's arithmetic

@pytest.mark.parametrize("in_node_nf", [9, 13, 2])
def test_restatement_agrees_with_the_oracle(in_node_nf):
    """The oracle runs in float64 here and takes the schedule values gamma; the restatement takes the coefficient rows rounded once to
    float32, like the kernel.  The two differ by that one rounding per coefficient (at most 3 * 2^-24 relative on a term), so they
    agree element by element within BOUND * U * A.  (The oracle in float32 is no yardstick for this: its sigma2_t|s is a difference of
    neighbouring softplus values and carries a relative error of 1e-3 at gamma_t - gamma_s = 0.001.)"""
    F = in_node_nf - 1
    rng = np.random.Generator(np.random.PCG64(in_node_nf))
    nm = np.zeros((4, 7), dtype=np.uint8)
    for b, idx in enumerate([range(7), range(4), [2], [0, 1, 3, 5, 6]]):
        nm[b, list(idx)] = 1
    B, N = nm.shape
    nmt = torch.from_numpy(nm.astype(np.float64))[:, :, None]
    emt = (nmt * nmt.transpose(1, 2) * (1 - torch.eye(N))).reshape(B * N * N, 1)
    sd_np = synthetic_state_dict(in_node_nf, 0, 32, 1, 2, True, 3, 1.0)
    cfg = orc.DynCfg(in_node_nf=in_node_nf, hidden_nf=32, n_layers=1)
    zt = rng.standard_normal((B, N, 3 + F)).astype(np.float32) * nm[:, :, None]
    zt[:, :, :3] += np.float32([3, -2, 1]) * nm[:, :, None]
    gamma_t = rng.uniform(-6.0, 8.0, size=B)
    gamma_s = gamma_t - rng.uniform(0.001, 0.5, size=B)
    gamma_0 = rng.uniform(-8.0, -4.0)
    t = torch.full((B, 1), 0.5)
    worst = {}
    for mol, rows in ((N, B), (N, 1), (5, B)):
        raw_x = rng.standard_normal((rows, mol, 3)).astype(np.float32)
        raw_h = rng.standard_normal((rows, mol, F)).astype(np.float32)
        raws = (torch.from_numpy(raw_x).double(), torch.from_numpy(raw_h).double())
        with orc.float64():
            sd = orc.as_torch_sd(sd_np)
            eps = orc.dynamics_forward(sd, cfg, t, zt, nmt, emt, None, None if mol == N else mol, prefix="dynamics.egnn.")
            zs = orc.posterior_step(sd, cfg, t, t, zt, nmt, emt, None, raws, mol_shape=None if mol == N else mol,
                                    gammas=(torch.from_numpy(gamma_s).view(B, 1), torch.from_numpy(gamma_t).view(B, 1)))
            assert zs.dtype == torch.float64 and torch.isfinite(eps).all()
            got, A = sr.posterior_step_ref(zt, eps.numpy(), sr.step_coef_rows(gamma_s, gamma_t), raw_x, raw_h, nm, mol)
            worst["step", mol, rows] = sr.ratio(got, zs.numpy(), A, nm)
            if mol < N:
                continue
            z, A = sr.noise_ref(raw_x, raw_h, nm)
            worst["noise", mol, rows] = sr.ratio(z, orc.combined_noise(raws[0], raws[1], nmt).numpy(), A, nm)
            eps0 = orc.dynamics_forward(sd, cfg, torch.zeros(B, 1), zt, nmt, emt, None, None, prefix="dynamics.egnn.")
            xo, ho = orc.final_decode(sd, cfg, zt, nmt, emt, None, raws, gamma_0=torch.full((B, 1), gamma_0, dtype=torch.float64))
            x, h, A = sr.final_decode_ref(zt, eps0.numpy(), sr.decode_coef3(gamma_0), raw_x, raw_h, nm)
            worst["decode", mol, rows] = sr.ratio(x, xo.numpy(), A, nm)
            assert np.array_equal(h, ho.numpy())
    for k, (r, nz) in worst.items():
        print(f"restatement vs float64 oracle, in_node_nf={in_node_nf} {k}: worst |err| / (2^-23 A) = {r:.3g}")
        assert r <= sr.BOUND and nz == 0, (k, r, nz)


def test_coefficient_rows_are_the_products():
    """step_coef_rows is noise_model.step_coefficients evaluated in float64."""
    from hierdiff_amd.noise_model import step_coefficients
    rng = np.random.Generator(np.random.PCG64(5))
    gt = rng.uniform(-6.0, 8.0, size=64)
    gs = gt - rng.uniform(0.001, 0.5, size=64)
    want = step_coefficients(torch.from_numpy(gs).view(-1, 1), torch.from_numpy(gt).view(-1, 1)).numpy()
    assert np.array_equal(sr.step_coef_rows(gs, gt), want)


# ----------------------------------------------------------------------------- the inputs keep the contract

@pytest.mark.parametrize("name", sr.STEP_CASES)
def test_case_inputs_keep_the_contract(name):
    c = CASES[name]
    masked = c["nm"] == 0
    for k in ("zt", "z0", "eps"):
        assert c[k].dtype == np.float32 and c[k].shape == (c["B"], c["N"], c["D"])
        assert np.all(c[k][masked] == 0), k
    assert np.all(c["z0_dirty"][:, :, :3] == c["z0"][:, :, :3]) and np.all(c["z0_dirty"][~masked] == c["z0"][~masked])
    assert c["nm"][:, :c["mol"]].sum(1).min() >= 1
    assert c["coef"].shape == (c["coef_rows"], 4) and c["raw_x"].shape == (c["noise_rows"], c["mol"], 3)
    assert c["raw_h"].shape == (c["noise_rows"], c["mol"], c["F"])
    if c["coef_rows"] > 1:
        assert len({tuple(r) for r in c["coef"]}) == c["B"]                # a different row per molecule
    off = (c["zt"][:, :, :3].sum(1) / c["nm"].sum(1)[:, None])
    assert np.all(np.abs(off) > 0.05), "zt carries a centre-of-mass offset"


# ----------------------------------------------------------------------------- float32 stays inside the bound; mutants leave it

def evaluate(entry, c, mutant=None, dirty=False):
    """(worst ratio over the valid elements, exact: masked elements are 0 and - decode - h has the reference's bits)."""
    nm = c["nm"]
    if entry == "noise":
        ref, A = sr.noise_ref(c["raw_x"], c["raw_h"], nm)
        r, nz = sr.ratio(sr.kernel_f32("noise", c, mutant), ref, A, nm)
        return r, nz == 0
    if entry == "step":
        ref, A = sr.posterior_step_ref(c["zt"], c["eps"], c["coef"], c["raw_x"], c["raw_h"], nm, c["mol"])
        r, nz = sr.ratio(sr.kernel_f32("step", c, mutant), ref, A, nm)
        return r, nz == 0
    z0 = c["z0_dirty"] if dirty else c["z0"]
    xr, hr, A = sr.final_decode_ref(z0, c["eps"], c["coef3"], c["raw_x"], c["raw_h"], nm)
    x, h = sr.kernel_f32("decode", c, mutant, z0=z0)
    r, _ = sr.ratio(x, xr, A, nm)
    return r, bool(np.array_equal(h.astype(np.float64), hr))


ENTRY_CASES = {"noise": sr.FULL_CASES, "step": sr.STEP_CASES, "decode": sr.FULL_CASES}


@pytest.mark.parametrize("entry", list(ENTRY_CASES))
def test_float32_evaluation_is_inside_the_bound(entry):
    for name in ENTRY_CASES[entry]:
        r, exact = evaluate(entry, CASES[name])
        print(f"float32 numpy {entry} [{name}]: worst |err| / (2^-23 A) = {r:.3g} (bound {sr.BOUND:g})")
        assert r <= sr.BOUND and exact, (entry, name, r, exact)
    if entry == "decode":
        for name in sr.FULL_CASES:
            r, exact = evaluate(entry, CASES[name], dirty=True)
            assert r <= sr.BOUND and exact, (entry, name, r, exact)


def _without(cases, *drop):
    return tuple(c for c in cases if c not in drop)


# mutant -> entry -> the cases in which it must be caught: those where it is not the identity.  In every other case of the entry the
# mutant must give the bits of the correct evaluation (asserted below), so the table cannot silently list too little.
MUST_CATCH = {
    "count_is_mol": {"noise": sr.FULL_CASES, "step": sr.STEP_CASES, "decode": sr.FULL_CASES},        # every case has a ragged molecule
    "no_final_recentre": {"step": sr.STEP_CASES},
    "ceps_without_alpha": {"step": sr.STEP_CASES},
    "coef_row_0_for_all": {"step": _without(sr.STEP_CASES, "S5")},                                      # S5 has one coefficient row
    "noise_row_0_for_all": {e: _without(cs, "S3") for e, cs in ENTRY_CASES.items()},                   # S3 has one noise row
    "noise_unmasked": dict(ENTRY_CASES),
    "decode_centres_eps": {"decode": sr.FULL_CASES},
    # z0 is zero at masked nodes (the contract), so there `h = z0[3:]` without the mask IS the identity; the mutant shows only on
    # z0_dirty, whose features are non-zero at masked nodes: a masked element of h that is not 0
    "decode_h_unmasked": {"decode_dirty": sr.FULL_CASES},
    "index_with_D_11": {e: ("S6", "S7") for e in ENTRY_CASES},
}


@pytest.mark.parametrize("mutant", sr.MUTANTS)
def test_every_mutant_is_rejected(mutant):
    table = MUST_CATCH[mutant]
    assert any(table.values()), "each mutant must be caught somewhere"
    for entry, names in ENTRY_CASES.items():
        for name in names:
            c = CASES[name]
            r, exact = evaluate(entry, c, mutant)
            if name in table.get(entry, ()):
                print(f"{mutant} {entry} [{name}]: worst ratio {r:.3g}, exact parts {'kept' if exact else 'broken'}")
                assert r > sr.BOUND, (mutant, entry, name, r)
            else:
                got, want = sr.kernel_f32(entry, c, mutant), sr.kernel_f32(entry, c)
                got, want = (got, want) if isinstance(got, tuple) else ((got,), (want,))
                assert all(np.array_equal(a, b) for a, b in zip(got, want)), (mutant, entry, name, "not listed, yet not the identity")
    for name in table.get("decode_dirty", ()):
        r, exact = evaluate("decode", CASES[name], mutant, dirty=True)
        assert not exact, (mutant, name)
