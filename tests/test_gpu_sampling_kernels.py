"""GPU tier (-m gpu): `k_noise`, `k_post_step` and `k_final_decode` (hd_noise, hd_posterior_step, hd_final_decode) on their own, called
at the C ABI on handles and topologies made through ctypes, against the float64 restatement of tests/sampling_reference.py on its
fixed cases: feature widths 1, 8 and 12, more than 64 nodes, element counts that are no multiple of 256, one coefficient / noise row
or one per molecule, `mol_shape < N`, masks that are no prefixes, and a `zt` with a centre-of-mass offset, which makes the final
re-centring count.

Bar: every valid element within BOUND * U * A = 8 * 2^-23 * A of float64, A the magnitude array of the restatement (derivation in
tests/sampling_reference.py, not fitted to what the kernels give); masked elements exactly 0.  The worst ratio |err| / (2^-23 A) of
every case is printed.  The output stage of the forward (`k_post1`, `k_post2`) at feature widths 12 and 1 and N = 70 is held to the
forward's own bar against the oracle."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import egnn_oracle as orc
from tests import sampling_reference as sr
from tests.helpers import assert_parity
from tests.test_gpu_parity import PRECISIONS

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = sr.cases()
SEED, BASE, DRAW = 99, 10, 2


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def make_config(F, H=32, L=1):
    from hierdiff_amd._lib import HdConfig
    return HdConfig(in_node_nf=F + 1, context_node_nf=0, n_dims=3, hidden_nf=H, n_layers=L, inv_sublayers=2, attention=1, tanh=1,
                    condition_time=1, norm_constant=0.0, normalization_factor=10.0, coords_range=30.0, precision=0, aggregation_mean=0)


@pytest.fixture(scope="module")
def lib():
    from hierdiff_amd import _lib
    _lib.require_gpu()
    return _lib.load()


@pytest.fixture(scope="module")
def handles(lib):
    """One handle per feature width.  hd_noise, hd_posterior_step and hd_final_decode read the handle's D and F and the topology's
    mask bytes only, no weights (step_launch, hd_final_decode, hd_noise in hierdiff_hip.hip): none are set."""
    made = {}
    for F in sorted({c["F"] for c in CASES.values()}):
        h = C.c_void_p()
        cfg = make_config(F)
        assert lib.hd_create(C.byref(cfg), 0, C.byref(h)) == 0, lib.hd_last_error()
        made[F] = h
    yield made
    torch.cuda.synchronize()
    for h in made.values():
        assert lib.hd_destroy(h) == 0


@contextlib.contextmanager
def topology(lib, h, nm):
    nm = np.ascontiguousarray(nm, dtype=np.uint8)
    t = C.c_void_p()
    assert lib.hd_topology_create(h, nm.ctypes.data, None, nm.shape[0], nm.shape[1], C.byref(t)) == 0, lib.hd_last_error()
    try:
        yield t
    finally:
        torch.cuda.synchronize()
        assert lib.hd_topology_destroy(t) == 0


def check(what, got, ref, A, nm):
    r, nonzero = sr.ratio(got, ref, A, nm)
    print(f"{what}: worst |err| / (2^-23 A) = {r:.3g} (bound {sr.BOUND:g})")
    assert np.all(np.isfinite(got)), what
    assert nonzero == 0, f"{what}: {nonzero} masked elements are not exactly 0"
    assert r <= sr.BOUND, f"{what}: ratio {r:.3g} > {sr.BOUND:g}"
    return r


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ----------------------------------------------------------------------------- hd_posterior_step

def device_step(lib, h, topo, c, in_place):
    zt, eps, coef, rx, rh = (dev(c[k]) for k in ("zt", "eps", "coef", "raw_x", "raw_h"))
    zs = zt if in_place else torch.full((c["B"], c["mol"], c["D"]), float("nan"), device=DEV)
    rc = lib.hd_posterior_step(h, topo, zt.data_ptr(), eps.data_ptr(), coef.data_ptr(), c["coef_rows"], rx.data_ptr(), rh.data_ptr(),
                               c["noise_rows"], c["mol"] if c["mol"] < c["N"] else -1, zs.data_ptr(), None)
    assert rc == 0, lib.hd_last_error()
    torch.cuda.synchronize()
    return zs.cpu().numpy()


@pytest.mark.parametrize("name", sr.STEP_CASES)
def test_posterior_step_against_float64(lib, handles, name):
    c = CASES[name]
    for k in ("zt", "eps"):
        assert np.all(c[k][c["nm"] == 0] == 0)                           # the contract: the inputs are zero at masked nodes
    ref, A = sr.posterior_step_ref(c["zt"], c["eps"], c["coef"], c["raw_x"], c["raw_h"], c["nm"], c["mol"])
    with topology(lib, handles[c["F"]], c["nm"]) as topo:
        zs = device_step(lib, handles[c["F"]], topo, c, in_place=False)
        assert zs.shape == ref.shape == (c["B"], c["mol"], c["D"])
        check(f"hd_posterior_step [{name}]", zs, ref, A, c["nm"])
        single = np.flatnonzero(c["nm"][:, :c["mol"]].sum(1) == 1)
        assert np.all(zs[single][:, :, :3] == 0), "the x row of a one-node molecule is exactly 0"
        assert single.size > 0 or name not in ("S1", "S2", "S6", "S8")
        if c["mol"] == c["N"]:
            assert np.array_equal(bits(device_step(lib, handles[c["F"]], topo, c, in_place=True)), bits(zs)), "zs == zt gives other bits"


# ----------------------------------------------------------------------------- hd_final_decode, hd_noise with injected normals

def device_decode(lib, h, topo, c, z0, raws, share=0, base=BASE):
    z0, eps = dev(z0), dev(c["eps"])
    B, N = z0.shape[:2]
    x = torch.full((B, N, 3), float("nan"), device=DEV)
    hf = torch.full((B, N, c["F"]), float("nan"), device=DEV)
    rx, rh = (None, None) if raws is None else (dev(raws[0]), dev(raws[1]))
    rc = lib.hd_final_decode(h, topo, z0.data_ptr(), eps.data_ptr(), (C.c_float * 3)(*[float(v) for v in c["coef3"]]),
                             None if rx is None else rx.data_ptr(), None if rh is None else rh.data_ptr(),
                             B if raws is None else raws[0].shape[0], SEED, base, DRAW, share, x.data_ptr(), hf.data_ptr(), None)
    assert rc == 0, lib.hd_last_error()
    torch.cuda.synchronize()
    return x.cpu().numpy(), hf.cpu().numpy()


def device_noise(lib, h, topo, c, raws, share=0, base=BASE, B=None):
    B = c["B"] if B is None else B
    z = torch.full((B, c["N"], c["D"]), float("nan"), device=DEV)
    rx, rh = (None, None) if raws is None else (dev(raws[0]), dev(raws[1]))
    rc = lib.hd_noise(h, topo, None if rx is None else rx.data_ptr(), None if rh is None else rh.data_ptr(),
                      B if raws is None else raws[0].shape[0], SEED, base, DRAW, share, z.data_ptr(), None)
    assert rc == 0, lib.hd_last_error()
    torch.cuda.synchronize()
    return z.cpu().numpy()


@pytest.mark.parametrize("name", sr.FULL_CASES)
def test_final_decode_against_float64(lib, handles, name):
    c = CASES[name]
    h = handles[c["F"]]
    m = (c["nm"] != 0).astype(np.float32)[:, :, None]
    with topology(lib, h, c["nm"]) as topo:
        for tag in ("z0", "z0_dirty"):                                   # z0_dirty: features that are not zero at masked nodes
            xr, hr, A = sr.final_decode_ref(c[tag], c["eps"], c["coef3"], c["raw_x"], c["raw_h"], c["nm"])
            x, hf = device_decode(lib, h, topo, c, c[tag], (c["raw_x"], c["raw_h"]))
            check(f"hd_final_decode x [{name}, {tag}, noise_rows {c['noise_rows']}]", x, xr, A, c["nm"])
            assert np.array_equal(bits(hf), bits(c[tag][:, :, 3:] * m)), "hfeat is z0[..., 3:] * m to the bit"
            assert np.array_equal(hf.astype(np.float64), hr) and np.all(hf[c["nm"] == 0] == 0)


@pytest.mark.parametrize("name", sr.FULL_CASES)
def test_noise_against_float64(lib, handles, name):
    c = CASES[name]
    ref, A = sr.noise_ref(c["raw_x"], c["raw_h"], c["nm"])
    with topology(lib, handles[c["F"]], c["nm"]) as topo:
        z = device_noise(lib, handles[c["F"]], topo, c, (c["raw_x"], c["raw_h"]))
    check(f"hd_noise [{name}, noise_rows {c['noise_rows']}]", z, ref, A, c["nm"])


# ----------------------------------------------------------------------------- the generator form (raw_x == NULL)

def host_normals(lib, c, rows, base):
    """[rows, N, 3] and [rows, N, F]: normal(seed, base + b, draw, n * D + c) from the library's host twin of the generator."""
    N, D = c["N"], c["D"]
    raw = np.array([[lib.hd_philox_normal_host(SEED, base + b, DRAW, i) for i in range(N * D)] for b in range(rows)],
                   dtype=np.float32).reshape(rows, N, D)
    return raw[:, :, :3].copy(), raw[:, :, 3:].copy()


@pytest.mark.parametrize("name", ["S1", "S3", "S6", "S7"])
def test_generator_form_of_noise_and_decode(lib, handles, name):
    c = CASES[name]
    h, nm, B = handles[c["F"]], c["nm"], c["B"]
    rx, rh = host_normals(lib, c, B, BASE)
    with topology(lib, h, nm) as topo:
        # one row per molecule, keyed by the global sample id
        z = device_noise(lib, h, topo, c, None)
        ref, A = sr.noise_ref(rx, rh, nm)
        check(f"hd_noise, generator [{name}]", z, ref, A, nm)
        x, hf = device_decode(lib, h, topo, c, c["z0"], None)
        xr, _, Ax = sr.final_decode_ref(c["z0"], c["eps"], c["coef3"], rx, rh, nm)
        check(f"hd_final_decode x, generator [{name}]", x, xr, Ax, nm)
        assert np.array_equal(bits(hf), bits(c["z0"][:, :, 3:]))
        # share_rows: the row of sample_id_base for every molecule
        zs = device_noise(lib, h, topo, c, None, share=1)
        ref, A = sr.noise_ref(rx[:1], rh[:1], nm)
        check(f"hd_noise, generator, share_rows [{name}]", zs, ref, A, nm)
        xs, _ = device_decode(lib, h, topo, c, c["z0"], None, share=1)
        xr, _, Ax = sr.final_decode_ref(c["z0"], c["eps"], c["coef3"], rx[:1], rh[:1], nm)
        check(f"hd_final_decode x, generator, share_rows [{name}]", xs, xr, Ax, nm)
    # a shard [lo, hi) drawn alone with base + lo gives the bits of its rows of the whole batch
    lo, hi = 1, B - 1
    sub = dict(c, B=hi - lo, eps=c["eps"][lo:hi])
    with topology(lib, h, nm[lo:hi]) as topo:
        assert np.array_equal(bits(device_noise(lib, h, topo, sub, None, base=BASE + lo)), bits(z[lo:hi]))
        xs, hs = device_decode(lib, h, topo, sub, c["z0"][lo:hi], None, base=BASE + lo)
        assert np.array_equal(bits(xs), bits(x[lo:hi])) and np.array_equal(bits(hs), bits(hf[lo:hi]))


# ----------------------------------------------------------------------------- the forward's output stage at other widths

@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("H", [32, 64])
@pytest.mark.parametrize("in_node_nf", [13, 2])
def test_output_stage_at_other_feature_widths(in_node_nf, H, precision):
    """F = 12 runs k_post1's second block of 8 outputs (4 of them past F), F = 1 a block with 7 past F; N = 70 the second node trip of
    k_post2.  The forward's own bar (tests/helpers.py) against the oracle."""
    from hierdiff_amd import EGNN_dynamics_QM9
    from hierdiff_amd.weights import synthetic_state_dict
    F = in_node_nf - 1
    sd_np = synthetic_state_dict(in_node_nf, 0, H, 1, 2, True, 7, 1.0)
    cfg = orc.DynCfg(in_node_nf=in_node_nf, hidden_nf=H, n_layers=1)
    xh, nm, em = orc.random_inputs([70, 9, 1], F, seed=11)
    t = torch.tensor([[0.3], [0.7], [0.1]])
    ref = orc.dynamics_forward(orc.as_torch_sd(sd_np), cfg, t, xh, nm, em, None, None, prefix="dynamics.egnn.").numpy()
    dyn = EGNN_dynamics_QM9(in_node_nf, 0, 3, hidden_nf=H, n_layers=1, attention=True, tanh=True, normalization_factor=10, inv_sublayers=2)
    dyn.load_numpy_state_dict(sd_np, prefix="dynamics.")
    dyn = dyn.to(DEV)
    dyn.precision = precision
    out = dyn._forward(t.to(DEV), xh.to(DEV), nm.to(DEV), em.to(DEV), None, None).cpu().numpy()
    assert out.shape == (3, 70, 3 + F)
    r, m = assert_parity(out, ref, f"forward F={F} H={H} [{precision}]")
    print(f"forward F={F} H={H} N=70 [{precision}]: rel_l2 {r:.2e} max_abs {m:.2e}")
    assert np.all(out[~nm.numpy()[..., 0]] == 0.0), "masked rows must be exactly zero"
    assert np.abs(ref[:, :, 3:]).max() > 1e-3                            # the feature columns carry signal


# ----------------------------------------------------------------------------- the step's LDS limit is refused on the host

def test_step_beyond_one_workgroups_lds_is_refused(lib):
    """mol * D floats of dynamic LDS: 1490 * 11 = 16,390 floats are 24 bytes past 64 KiB.  Refused before any launch, in the words of
    hd_multistep_step; the pocket form of the same topology, whose molecule part fits, runs."""
    from hierdiff_amd.weights import flatten_dynamics, synthetic_state_dict
    B, N, D, F = 1, 1490, 11, 8
    h = C.c_void_p()
    cfg = make_config(F)
    assert lib.hd_create(C.byref(cfg), 0, C.byref(h)) == 0, lib.hd_last_error()
    assert N * D * 4 > 64 * 1024 >= (N - 1) * D * 4
    nm = np.zeros((B, N), dtype=np.uint8)
    nm[0, :2] = 1
    z = torch.zeros(B, N, D, device=DEV)
    out = torch.full((B, N, D), float("nan"), device=DEV)
    coef = dev(sr.step_coef_rows([0.5], [1.0]))
    rx, rh = torch.zeros(B, N, 3, device=DEV), torch.zeros(B, N, F, device=DEV)
    with topology(lib, h, nm) as topo:
        step = lambda mol, zs: lib.hd_posterior_step(h, topo, z.data_ptr(), z.data_ptr(), coef.data_ptr(), 1, rx.data_ptr(), rh.data_ptr(),
                                                     1, mol, zs.data_ptr(), None)
        for mol in (-1, N):
            assert step(mol, out) == -1
            msg = lib.hd_last_error()
            assert b"hd_posterior_step" in msg and b"N * D floats exceed one workgroup's LDS" in msg, msg
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all()), "a refused call writes nothing"
        assert step(N - 1, out) == 0, lib.hd_last_error()                # 65,516 bytes: the largest molecule part that fits
        torch.cuda.synchronize()
        assert bool((out[:, :N - 1] == 0).all()) and bool(torch.isnan(out.view(-1)[(N - 1) * D:]).all())
        # the loops that launch the same kernel: weights, a two-step schedule and a one-transition path are enough to be asked
        n = lib.hd_weight_count(h)
        blob = np.ascontiguousarray(flatten_dynamics(synthetic_state_dict(F + 1, 0, 32, 1), F + 1, 0, 32, 1, 2, True, prefix="dynamics."))
        assert blob.size == n and blob.dtype == np.float32
        assert lib.hd_set_weights(h, blob.ctypes.data, n, 0, None) == 0, lib.hd_last_error()
        rows = sr.step_coef_rows([0.5, 1.0], [1.0, 1.5])
        assert lib.hd_set_schedule(h, 2, (C.c_float * 3)(0.0, 0.5, 1.0), rows.ctypes.data_as(C.POINTER(C.c_float))) == 0, lib.hd_last_error()
        assert lib.hd_set_path(h, 1, (C.c_int * 1)(2), (C.c_int * 1)(0), rows.ctypes.data_as(C.POINTER(C.c_float)), 0, None) == 0, lib.hd_last_error()
        assert lib.hd_sample_loop(h, topo, z.data_ptr(), None, -1, 2, 0, None, None, 1, SEED, BASE, 0, None) == -1
        msg = lib.hd_last_error()
        assert b"hd_sample_loop" in msg and b"N * D floats exceed one workgroup's LDS" in msg, msg
        assert lib.hd_sample_path(h, topo, z.data_ptr(), None, -1, 0, 1, None, None, 1, SEED, BASE, 0, None) == -1
        msg = lib.hd_last_error()
        assert b"hd_sample_path" in msg and b"N * D floats exceed one workgroup's LDS" in msg, msg
        torch.cuda.synchronize()
        assert bool((z == 0).all())
    assert lib.hd_destroy(h) == 0
