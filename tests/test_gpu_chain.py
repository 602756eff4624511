"""GPU tier (-m gpu) of recorded trajectories (`sample_chain`; hd_set_chain, hd_chain_attach, k_chain_frame): the frames a path loop
writes while it runs against the same chain cut into single transitions (`path_steps` / `inpaint_steps` / `latent_steps`, which the
few-step, inpainting, editing, guidance and solver tiers hold piece-wise bit-identical to the whole), with `unnormalize` applied in
torch on the device.  Every comparison of a state is `torch.equal`; the data prediction (record="x0") is held to the element-wise
bar of tests/test_gpu_sampling_kernels.py against float64.

The small synthetic model of the few-step and solver tiers (H = 32, 2 layers, T = 20) on B = 3 molecules of sizes 5, 4 and 1 padded
to N = 5: a full row, a padded row and a single-node molecule."""
import pytest
import torch

from oracle import egnn_oracle as orc
from tests.test_gpu_fewstep import context_for, dev, make_model

pytestmark = pytest.mark.gpu

H, L, T = 32, 2, 20
SIZES = [5, 4, 1]
BASE = 10
K_FEW, KEEP_FEW = 6, 4
ULP = 2.0 ** -23


def masks():
    nm, em = orc.canonical_masks(SIZES)
    return dev(nm.bool()), em


def start_state(nm, seed):
    """[B,N,11] normals on the device: masked, the x part mean-free over the valid nodes."""
    g = torch.Generator().manual_seed(seed)
    B, N = nm.shape[:2]
    rx, rh = torch.randn(B, N, 3, generator=g), torch.randn(B, N, 8, generator=g)
    return dev(orc.combined_noise(rx, rh, nm.cpu().float()))


def unnorm(model, z, nm):
    """`model.unnormalize` in torch on the device, as one [B,N,D] tensor."""
    x, h = model.unnormalize(z[:, :, :3], z[:, :, 3:], nm.to(z.dtype))
    return torch.cat([x, h], dim=2)


def cut_chain(step, z, K):
    """states[p], p = K .. 0 counted from the t = 0 end: `step(z, k)` is transition k alone."""
    states = {K: z}
    for k in range(K):
        states[K - 1 - k] = step(states[K - k], k)
    return states


def last_write_wins(model, states, K, keep, nm):
    """The reference's loop replayed over the single-step states: chain[(p * keep) // K] = z_p, later writes win."""
    frames = [None] * keep
    for p in reversed(range(K)):
        frames[(p * keep) // K] = unnorm(model, states[p], nm)
    return frames


def check_frames(chain, frames, x, h, what):
    assert chain.shape[0] == len(frames), what
    assert torch.equal(chain[0], torch.cat([x, h], dim=2)), f"{what}: frame 0 is not the decode"
    for f in range(1, len(frames)):
        assert torch.equal(chain[f], frames[f]), f"{what}: frame {f}"


@pytest.fixture(scope="module")
def small():
    """The model, its masks, z_T and the T single-transition states of the identity path below it (computed once, never changed)."""
    model, _, _ = make_model(H, L, T)
    nm, _ = masks()
    zT = start_state(nm, 1)
    states = cut_chain(lambda z, k: model.path_steps(z, nm, k_lo=k, k_hi=k + 1, sample_id_base=BASE), zT, T)
    plain = model.sample_from_masks(nm, None, None, sample_id_base=BASE, z_init=zT)
    return model, nm, zT, states, plain


# ----------------------------------------------------------------------------- 1 / 2. the identity path

def test_identity_path_keeps_every_state(small):
    model, nm, zT, states, plain = small
    x, h, chain = model.sample_from_masks(nm, None, None, sample_id_base=BASE, z_init=zT, keep_frames=T)
    assert tuple(chain.shape) == (T, 3, 5, 11) and chain.is_cuda
    assert torch.equal(x, plain[0]) and torch.equal(h, plain[1])
    check_frames(chain, [unnorm(model, states[f], nm) for f in range(T)], plain[0], plain[1], "keep = T")


def test_keep_7_of_20_is_last_write_wins(small):
    model, nm, zT, states, plain = small
    x, h, chain = model.sample_from_masks(nm, None, None, sample_id_base=BASE, z_init=zT, keep_frames=7)
    assert torch.equal(x, plain[0]) and torch.equal(h, plain[1])
    check_frames(chain, last_write_wins(model, states, T, 7, nm), plain[0], plain[1], "keep = 7")


def test_sample_chain_entry_point(small):
    from hierdiff_amd import EnVariationalDiffusion
    model, nm, zT, states, plain = small
    flat = EnVariationalDiffusion.sample_chain(model, 3, 5, nm, None, None, keep_frames=5)
    want = model.sample_from_masks(nm, None, None, keep_frames=5)
    full = EnVariationalDiffusion.sample_chain(model, 3, 5, nm, None, None)
    assert tuple(flat.shape) == (15, 5, 11) and tuple(full.shape) == (3 * T, 5, 11)
    assert torch.equal(flat, want[2].reshape(15, 5, 11))
    assert torch.equal(flat[:3], torch.cat([want[0], want[1]], dim=2))


# ----------------------------------------------------------------------------- 3. few-step chains of every kind

@pytest.mark.parametrize("few", [dict(eta=0.0), dict(eta=1.0), dict(solver="dpm2m")], ids=["eta0", "eta1", "dpm2m"])
def test_few_step_chain(small, few):
    model, nm, zT, _, _ = small
    states = cut_chain(lambda z, k: model.path_steps(z, nm, steps=K_FEW, k_lo=k, k_hi=k + 1, sample_id_base=BASE, **few), zT, K_FEW)
    plain = model.sample_from_masks(nm, None, None, sample_id_base=BASE, z_init=zT, steps=K_FEW, **few)
    x, h, chain = model.sample_from_masks(nm, None, None, sample_id_base=BASE, z_init=zT, steps=K_FEW, keep_frames=KEEP_FEW, **few)
    assert torch.equal(x, plain[0]) and torch.equal(h, plain[1])
    check_frames(chain, last_write_wins(model, states, K_FEW, KEEP_FEW, nm), plain[0], plain[1], str(few))


def test_guided_chain():
    model, _, _ = make_model(H, L, T, C_=1)
    nm, _ = masks()
    ctx = dev(context_for(nm.cpu()))
    zT = start_state(nm, 2)
    kw = dict(steps=K_FEW, guidance_scale=2.0, sample_id_base=BASE)
    states = cut_chain(lambda z, k: model.path_steps(z, nm, None, ctx, k_lo=k, k_hi=k + 1, **kw), zT, K_FEW)
    plain = model.sample_from_masks(nm, None, ctx, z_init=zT, **kw)
    x, h, chain = model.sample_from_masks(nm, None, ctx, z_init=zT, keep_frames=KEEP_FEW, **kw)
    assert torch.equal(x, plain[0]) and torch.equal(h, plain[1])
    check_frames(chain, last_write_wins(model, states, K_FEW, KEEP_FEW, nm), plain[0], plain[1], "guided")


def test_inpainting_chain_keeps_the_state_after_the_last_round(small):
    from hierdiff_amd import _lib
    from hierdiff_amd.diffusion import _stream
    model, nm, _, _, _ = small
    B, N = nm.shape[:2]
    fm = torch.zeros(B, N, 1, dtype=torch.bool)
    fm[0, :2] = True
    fm[1, :1] = True
    fm = dev(fm)
    g = torch.Generator().manual_seed(5)
    xk, hk = dev(torch.randn(B, N, 3, generator=g)), dev(torch.randn(B, N, 8, generator=g))
    model.sample_steps = K_FEW                         # `inpaint_steps` takes its path from the model's attributes
    try:
        zT = torch.empty(B, N, 11, device=nm.device)
        topo = model.dynamics.topology(nm, None, B, N)
        _lib.check(_lib.load().hd_noise(model._lib_handle(), topo.ptr, None, None, B, model.seed, BASE, 0, 0, zT.data_ptr(),
                                        _stream(nm.device)), "hd_noise")
        states = cut_chain(lambda z, k: model.inpaint_steps(z, K_FEW - k, K_FEW - k - 1, nm, fm, xk, hk, resamplings=2,
                                                            sample_id_base=BASE), zT, K_FEW)
        plain = model.sample_inpaint(nm, fm, xk, hk, resamplings=2, sample_id_base=BASE)
        x, h, chain = model.sample_inpaint(nm, fm, xk, hk, resamplings=2, sample_id_base=BASE, keep_frames=KEEP_FEW)
    finally:
        model.sample_steps = None
    assert torch.equal(x, plain[0]) and torch.equal(h, plain[1])
    check_frames(chain, last_write_wins(model, states, K_FEW, KEEP_FEW, nm), plain[0], plain[1], "inpainting")


def test_chain_from_a_latent(small):
    model, nm, zT, _, _ = small
    kw = dict(t_start=12, steps=K_FEW, sample_id_base=BASE)
    states = cut_chain(lambda z, k: model.latent_steps(z, nm, k_lo=k, k_hi=k + 1, **kw), zT, K_FEW)
    plain = model.sample_from_latent(zT, nm, **kw)
    x, h, chain = model.sample_from_latent(zT, nm, keep_frames=KEEP_FEW, **kw)
    assert torch.equal(x, plain[0]) and torch.equal(h, plain[1])
    check_frames(chain, last_write_wins(model, states, K_FEW, KEEP_FEW, nm), plain[0], plain[1], "latent")


# ----------------------------------------------------------------------------- 4. non-unit normalisation

def test_frames_are_unnormalised_like_torch_and_padded_rows_are_zero():
    model, _, _ = make_model(H, L, T)
    model.norm_values, model.norm_biases, model._unit_norm = [2.0, 0.25, 1.0], [None, 0.5, 0.0], False
    nm, _ = masks()
    zT = start_state(nm, 3)
    states = cut_chain(lambda z, k: model.path_steps(z, nm, steps=K_FEW, k_lo=k, k_hi=k + 1, sample_id_base=BASE), zT, K_FEW)
    plain = model.sample_from_masks(nm, None, None, sample_id_base=BASE, z_init=zT, steps=K_FEW)
    x, h, chain = model.sample_from_masks(nm, None, None, sample_id_base=BASE, z_init=zT, steps=K_FEW, keep_frames=K_FEW)
    assert torch.equal(x, plain[0]) and torch.equal(h, plain[1])
    frames = last_write_wins(model, states, K_FEW, K_FEW, nm)
    check_frames(chain, frames, plain[0], plain[1], "norm_values (2, 0.25), bias 0.5")
    assert float(frames[1][:, :, 3:].abs().max()) > 0.5 and not torch.equal(frames[1], states[1])     # the test is not vacuous
    pad = ~nm.expand_as(chain[0])
    for f in range(1, K_FEW):
        assert torch.all(chain[f][pad] == 0), f"frame {f}: padded rows"


# ----------------------------------------------------------------------------- 5. plain launches

@pytest.mark.parametrize("few", [dict(), dict(steps=K_FEW, solver="dpm2m")], ids=["identity", "dpm2m"])
def test_plain_launches_give_the_frames_of_the_graph(small, few):
    model, nm, zT, _, _ = small
    keep = 7 if not few else KEEP_FEW
    a = model.sample_from_masks(nm, None, None, sample_id_base=BASE, z_init=zT, keep_frames=keep, **few)
    model.use_graph = False
    try:
        b = model.sample_from_masks(nm, None, None, sample_id_base=BASE, z_init=zT, keep_frames=keep, **few)
    finally:
        model.use_graph = True
    for u, v in zip(a, b):
        assert torch.equal(u, v)


# ----------------------------------------------------------------------------- 6. the graph slot

def test_graph_build_counters():
    from hierdiff_amd import _lib
    lib = _lib.load()
    nm, _ = masks()
    zT = start_state(nm, 4)
    model, _, _ = make_model(H, L, T)
    fresh, _, _ = make_model(H, L, T)                  # never records
    call = lambda m, **kw: m.sample_from_masks(nm, None, None, sample_id_base=BASE, z_init=zT, steps=K_FEW, **kw)
    topo = model.dynamics.topology(nm, None, 3, 5)
    counters = lambda t: (lib.hd_path_graph_builds(t.ptr), lib.hd_guided_graph_builds(t.ptr), lib.hd_chain_graph_builds(t.ptr))
    assert counters(topo) == (0, 0, 0)
    first = call(model, keep_frames=KEEP_FEW)
    assert counters(topo) == (0, 0, 1)
    second = call(model, keep_frames=KEEP_FEW)         # a new sink tensor: the pointer is not baked into the graph
    assert first[2].data_ptr() != second[2].data_ptr() and torch.equal(first[2], second[2])
    assert counters(topo) == (0, 0, 1)
    plain = call(model)
    assert counters(topo) == (1, 0, 1)
    for _ in range(2):                                 # recording and plain calls alternate: nothing is evicted
        again = call(model, keep_frames=KEEP_FEW)
        assert torch.equal(again[2], first[2])
        assert torch.equal(call(model)[0], plain[0])
    assert counters(topo) == (1, 0, 1)
    # behind the detach a plain call is that of a topology that never recorded
    want = call(fresh)
    assert torch.equal(plain[0], want[0]) and torch.equal(plain[1], want[1])
    assert counters(fresh.dynamics.topology(nm, None, 3, 5)) == (1, 0, 0)
    # another frame table is another graph; the same one again is not
    call(model, keep_frames=3)
    assert counters(topo) == (1, 0, 2)


def test_guided_recording_does_not_touch_the_guided_slot():
    from hierdiff_amd import _lib
    lib = _lib.load()
    model, _, _ = make_model(H, L, T, C_=1)
    nm, _ = masks()
    ctx = dev(context_for(nm.cpu()))
    topo = model.dynamics.topology(nm, None, 3, 5)
    kw = dict(steps=K_FEW, guidance_scale=2.0, sample_id_base=BASE)
    plain = model.sample_from_masks(nm, None, ctx, **kw)
    before = (lib.hd_path_graph_builds(topo.ptr), lib.hd_guided_graph_builds(topo.ptr))
    assert before == (0, 1)
    rec = model.sample_from_masks(nm, None, ctx, keep_frames=KEEP_FEW, **kw)
    again = model.sample_from_masks(nm, None, ctx, **kw)
    assert (lib.hd_path_graph_builds(topo.ptr), lib.hd_guided_graph_builds(topo.ptr)) == before
    assert lib.hd_chain_graph_builds(topo.ptr) == 1
    assert torch.equal(rec[0], plain[0]) and torch.equal(again[0], plain[0])


# ----------------------------------------------------------------------------- 7. a molecule's frames depend on its global id only

def test_frames_depend_on_the_global_id_only(small):
    model, nm, _, _, _ = small
    whole = model.sample_from_masks(nm, None, None, sample_id_base=BASE, steps=K_FEW, keep_frames=KEEP_FEW)
    alone = model.sample_from_masks(nm[1:2].contiguous(), None, None, sample_id_base=BASE + 1, steps=K_FEW, keep_frames=KEEP_FEW)
    assert torch.equal(whole[2][:, 1], alone[2][:, 0])
    assert torch.equal(whole[0][1], alone[0][0]) and torch.equal(whole[1][1], alone[1][0])


# ----------------------------------------------------------------------------- 8. the data prediction against float64

@pytest.mark.parametrize("few", [dict(), dict(steps=K_FEW, eta=0.0)], ids=["identity", "eta0"])
def test_x0_frames_against_float64(small, few):
    """Every element within 8 * 2^-23 * (|z_t| + sigma_t |eps^|) / alpha_t of the float64 value of (z_t - sigma_t eps^) / alpha_t.
    Measured on an MI355X: at most 1.071 (identity path) and 0.999 (K = 6, eta = 0) of those 8."""
    from hierdiff_amd import paths
    model, nm, zT, ident, _ = small
    K = few.get("steps", T)
    path = paths.build_path(T, K)
    states = ident if not few else cut_chain(
        lambda z, k: model.path_steps(z, nm, k_lo=k, k_hi=k + 1, sample_id_base=BASE, **few), zT, K)
    plain = model.sample_from_masks(nm, None, None, sample_id_base=BASE, z_init=zT, **few)
    x, h, chain = model.sample_from_masks(nm, None, None, sample_id_base=BASE, z_init=zT, keep_frames=K, record="x0", **few)
    assert torch.equal(x, plain[0]) and torch.equal(h, plain[1])
    assert torch.equal(chain[0], torch.cat([x, h], dim=2))
    tabs = model._schedule(rows=3)
    topo = model.dynamics.topology(nm, None, 3, 5)
    cf = paths.chain_frames(K, K, path)
    worst, checked = 0.0, 0
    for k, f in enumerate(cf.frame_of):
        if f == 0:
            continue                                   # overwritten by the decode
        t = path[k]
        alpha, sigma = model._alpha_sigma(tabs, t)
        zt = states[K - k]
        tt = torch.full((3, 1), float(tabs["tau"][t]), device=zt.device)
        eps = model.dynamics.forward_with_topology(topo, tt, zt, None, None)
        zt64, e64 = zt.double(), eps.double()
        want = (zt64 - sigma * e64) / alpha
        scale = (zt64.abs() + sigma * e64.abs()) / alpha
        err = (chain[f].double() - want).abs()
        assert bool((err <= 8 * ULP * scale).all()), f"transition {k} (t = {t}): {float((err / (ULP * scale).clamp(min=1e-300)).max()):.2f} x 2^-23"
        ok = scale > 0
        worst = max(worst, float((err[ok] / (ULP * scale[ok])).max()))
        checked += err.numel()
    assert checked == (K - 1) * 3 * 5 * 11             # no element left out
    print(f"record='x0' {few or 'identity path'}: worst error {worst:.3f} x 2^-23 (|z_t| + sigma_t |eps^|) / alpha_t over {checked} elements (bar 8)")


# ----------------------------------------------------------------------------- 9. refusals leave no sink attached

def test_refusals_leave_no_sink_attached(small):
    from hierdiff_amd import _lib
    lib = _lib.load()
    model, nm, zT, _, _ = small
    call = lambda **kw: model.sample_from_masks(nm, None, None, sample_id_base=BASE, z_init=zT, steps=K_FEW, **kw)
    topo = model.dynamics.topology(nm, None, 3, 5)
    want = call()
    before = (lib.hd_path_graph_builds(topo.ptr), lib.hd_chain_graph_builds(topo.ptr))
    for bad in (dict(keep_frames=K_FEW + 1), dict(keep_frames=0), dict(record="x0"), dict(keep_frames=2, record="eps")):
        with pytest.raises(ValueError):
            call(**bad)
    with pytest.raises(NotImplementedError, match="pocket"):
        call(keep_frames=2, pocket=(None,) * 4)
    model.noise_mode = "torch"
    try:
        with pytest.raises(NotImplementedError, match="noise_mode"):
            model.sample_from_masks(nm, None, None, steps=K_FEW, keep_frames=2)
    finally:
        model.noise_mode = "philox"
    model.dynamics.mode = "gnn_dynamics"
    try:
        with pytest.raises(NotImplementedError, match="gnn_dynamics"):
            call(keep_frames=2)
    finally:
        model.dynamics.mode = "egnn_dynamics"
    # the C ABI's own refusals: a frame outside the sink, a K other than the path's, a sink of another size than the tables
    import ctypes as C
    fo = (C.c_int * K_FEW)(*([0] * K_FEW))
    fo[0] = 4
    assert lib.hd_set_chain(model._lib_handle(), K_FEW, fo, None, 4) == -1 and b"frame_of" in lib.hd_last_error()
    assert lib.hd_set_chain(model._lib_handle(), K_FEW - 1, fo, None, 8) == -1 and b"K differs" in lib.hd_last_error()
    got = call()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert (lib.hd_path_graph_builds(topo.ptr), lib.hd_chain_graph_builds(topo.ptr)) == before


# ----------------------------------------------------------------------------- the list level

def test_results_carry_their_chain(small):
    model, nm, _, _, _ = small
    torch.manual_seed(0)
    plain = model.sample(3, "cuda:0", sample_id_base=BASE, steps=K_FEW)
    torch.manual_seed(0)
    res = model.sample(3, "cuda:0", sample_id_base=BASE, steps=K_FEW, keep_frames=KEEP_FEW)
    for a, b in zip(plain, res):
        n = a["x"].shape[0]
        assert torch.equal(a["x"], b["x"]) and torch.equal(a["h"], b["h"])
        assert tuple(b["chain_x"].shape) == (KEEP_FEW, n, 3) and tuple(b["chain_h"].shape) == (KEEP_FEW, n, 8)
        assert not b["chain_x"].is_cuda and torch.equal(b["chain_x"][0], b["x"]) and torch.equal(b["chain_h"][0], b["h"])
        assert b["chain_t"].tolist() == model._chain_times(KEEP_FEW, steps=K_FEW).tolist()
        assert "chain_x" not in a
