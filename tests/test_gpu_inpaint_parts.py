"""GPU tier (-m gpu) of partial inpainting - positions or features alone, per channel (hd_inpaint_parts, hd_inpaint_replace,
hd_inpaint_decode_fix_parts; `fixed_x_mask` / `fixed_h_mask` of sample_inpaint / inpaint_steps, the partial entries of sample_grow,
--known-parts): the replacement kernel against the float64 restatement of tests/inpaint_parts_reference.py, the bit identities
with the whole-node call, chains against the restatement over the oracle, what comes back, locality, graphs and the command line.

Bars.  hd_inpaint_replace: the element-wise bar of tests/sampling_reference.py - every element within 8 * 2^-23 of the sum of the
absolute values of its terms (`replace_parts_mag`); tests/test_inpaint_parts_cpu.py shows the fp32 restatement below 0.1 of it and
every mutant above 1e5 of it on these inputs.  Chains: REL_L2_TOL / MAX_ABS_TOL of tests/helpers.py per state.  Measured figures
are printed.  Shapes: the kernel at B = 7, N in {5, 33}, F in {1, 8}; chains at H = 32 (fixture f7_h32_l2) and T = 8."""
import ctypes as C
import pickle

import numpy as np
import pytest
import torch

from hierdiff_amd import _lib, paths
from hierdiff_amd.restraints import Field, Restraints
from oracle import egnn_oracle as orc
from tests import edit_reference as er
from tests import guidance_reference as gr
from tests import inpaint_parts_reference as pr
from tests import restraint_frame_reference as fr
from tests import restraint_reference as rr
from tests.helpers import MAX_ABS_TOL, REL_L2_TOL, fixture_model, load, rel_l2
from tests.test_gpu_inpaint import DEV, FIXTURE, dev, errors, make_case, make_model
from tests.test_gpu_restraint import Bare, stream
from tests.test_inpaint_cpu import SEED, gamma_grid_fp64, philox_raw

pytestmark = pytest.mark.gpu

T = 8
BOTH = ["fp32", "fp16x3"]


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def u8(mask):
    return dev(mask.reshape(-1).to(torch.uint8)).contiguous()


def replace(bare, c, z, fx, fh, draw=None):
    """hd_inpaint_replace in place on a device copy of z; fh None: the whole-node form."""
    zd, kd, fxd = dev(z).clone().contiguous(), dev(c.known).contiguous(), u8(fx)
    fhd = None if fh is None else u8(fh)
    rc = bare.lib.hd_inpaint_replace(bare.h, bare.topo, zd.data_ptr(), fxd.data_ptr(), None if fhd is None else fhd.data_ptr(),
                                     kd.data_ptr(), c.alpha, c.sigma, c.seed, c.base, c.draw if draw is None else draw, stream())
    assert rc == 0, bare.lib.hd_last_error()
    return zd.cpu()


# ----------------------------------------------------------------------------- 1. the kernel against float64

@pytest.mark.parametrize("N,F", pr.KERNEL_SHAPES)
def test_inpaint_replace_against_float64(lib, N, F):
    c = pr.kernel_case(N, F)
    bare = Bare(c.D, c.nm)
    try:
        ids = [c.base + b for b in range(c.B)]
        raw = philox_raw(lib, c.seed, ids, c.draw, N, F)              # the generator's host twin
        nm = c.nm[:, :, None]
        ref = pr.replace_parts_ref(c.z.double(), c.known.double(), nm, c.fx, c.fh, c.alpha, c.sigma, tuple(r.double() for r in raw))
        mag = pr.replace_parts_mag(c.z, c.known, nm, c.fx, c.fh, c.alpha, c.sigma, raw)
        got = replace(bare, c, c.z, c.fx, c.fh)
        ratio = pr.kernel_ratio(got.numpy(), ref.numpy(), mag.numpy())
        print(f"hd_inpaint_replace N={N} F={F}: worst err / bound {ratio:.3f} (1.0 = 8 units of 2^-23 sum|terms|)")
        assert ratio <= 1.0
        bits = lambda t: t.contiguous().numpy().view(np.uint32)
        assert (bits(got[0]) == bits(c.z[0])).all()                               # nothing fixed: z_gen bit for bit
        assert (bits(got[2][:, :3]) == bits(c.z[2][:, :3])).all()                 # |Fx| = 0: the position part keeps its bits
        assert not torch.equal(got[2][:, 3:], c.z[2][:, 3:])
        assert (bits(got[~c.nm]) == bits(c.z[~c.nm])).all()                       # masked rows (bytes set, garbage known) untouched
        assert torch.isfinite(got).all()
        free = ~(c.fh & nm)
        assert (bits(got[:, :, 3:][free]) == bits(c.z[:, :, 3:][free])).all()     # a channel that is not replaced keeps its bits
        assert float((got[:, :, :3] * nm).sum(1).abs().max()) < 1e-5 * float(got[:, :, :3].abs().max())
        # coinciding masks: the bits of the whole-node instantiation
        for fm in (c.fx, c.fh.any(2), c.nm.clone(), torch.zeros_like(c.fx)):
            whole = replace(bare, c, c.z, fm, None)
            parts = replace(bare, c, c.z, fm, fm[:, :, None].expand(c.B, N, F))
            assert (bits(whole) == bits(parts)).all()
        # positions only: the features keep their bits; another draw gives other normals
        xo = replace(bare, c, c.z, c.fx, torch.zeros_like(c.fh))
        assert (bits(xo[:, :, 3:]) == bits(c.z[:, :, 3:])).all() and not torch.equal(xo[:, :, :3], c.z[:, :, :3])
        assert not torch.equal(replace(bare, c, c.z, c.fx, c.fh, draw=c.draw + 1), got)
        # refusals, worded under the entry point's own name
        zd = dev(c.z).clone()
        assert lib.hd_inpaint_replace(bare.h, bare.topo, zd.data_ptr(), None, None, zd.data_ptr(), 0.8, 0.6, 0, 0, 0, stream()) == -1
        assert b"hd_inpaint_replace" in lib.hd_last_error()
        assert lib.hd_inpaint_parts(bare.h, None, None, stream()) == -1 and b"hd_inpaint_parts" in lib.hd_last_error()
    finally:
        bare.close()


def test_decode_fix_parts_bits():
    c = pr.kernel_case(33, 8)
    bare = Bare(c.D, c.nm)
    try:
        g = torch.Generator().manual_seed(3)
        x, h = torch.randn(c.B, 33, 3, generator=g), torch.randn(c.B, 33, 8, generator=g)
        xk, hk = (c.known[:, :, :3] * pr.NV0).contiguous(), c.known[:, :, 3:].contiguous()
        xd, hd, xkd, hkd, fxd, fhd = dev(x).clone(), dev(h).clone(), dev(xk), dev(hk), u8(c.fx), u8(c.fh)
        rc = bare.lib.hd_inpaint_decode_fix_parts(bare.h, bare.topo, fxd.data_ptr(), fhd.data_ptr(), xkd.data_ptr(), hkd.data_ptr(),
                                                  xd.data_ptr(), hd.data_ptr(), stream())
        assert rc == 0, bare.lib.hd_last_error()
        xg, hg = xd.cpu(), hd.cpu()
        nm = c.nm[:, :, None]
        rep, fxv = c.fh & nm, c.fx & c.nm
        assert torch.equal(hg[rep], hk[rep]) and torch.equal(hg[~rep], h[~rep])   # h_known exactly; every other element's bits
        assert torch.equal(xg[~fxv], x[~fxv])
        xr, _ = pr.decode_fix_parts_ref(x.double(), h.double(), xk.double(), hk.double(), nm, c.fx, c.fh)
        tol = 4 * 2.0 ** -23 * (x.abs().max() + xk.abs().max())
        assert float((xg.double() - xr).abs().max()) <= tol
        for b in (1, 3, 4, 6):                                                    # the block comes back as a pure translation
            d = (xg - xk)[b][fxv[b]]
            assert float((d - d[0]).abs().max()) <= 2 * float(np.spacing(np.float32(max(xg[b].abs().max(), xk[b][c.nm[b]].abs().max()))))
        # coinciding masks: the whole-node fix-up's bits
        fmd, fmFd = u8(c.fx), u8(c.fx[:, :, None].expand(c.B, 33, 8))
        outs = []
        for parts in (False, True):
            xd, hd = dev(x).clone(), dev(h).clone()
            if parts:
                rc = bare.lib.hd_inpaint_decode_fix_parts(bare.h, bare.topo, fmd.data_ptr(), fmFd.data_ptr(), xkd.data_ptr(), hkd.data_ptr(),
                                                          xd.data_ptr(), hd.data_ptr(), stream())
            else:
                rc = bare.lib.hd_inpaint_decode_fix(bare.h, bare.topo, fmd.data_ptr(), xkd.data_ptr(), hkd.data_ptr(), xd.data_ptr(),
                                                    hd.data_ptr(), stream())
            assert rc == 0
            outs.append((xd.cpu(), hd.cpu()))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    finally:
        bare.close()


# ----------------------------------------------------------------------------- the masks of the model-level tests

MASKS = ("h_only", "x_only", "mixed")


def parts_case(kind, C_=0, seed=0):
    """tests/test_gpu_inpaint.py's molecules (8, 5, 7, 3, 6 nodes; 0, 1, 3, 3, 6 of them known) with the knowledge cut to the
    features, to the positions, or mixed: the channels of pr.CHANNELS on the known nodes and on the first free one, the position
    of every known node but the first of molecules 2 and 4 (known features, free position)."""
    nm, em, fm, xk, hk, ctx = make_case(C_=C_, seed=seed)
    B, N = nm.shape[:2]
    fx, fh = fm.clone(), fm.expand(B, N, 8).clone()
    if kind == "h_only":
        fx[:] = False
    elif kind == "x_only":
        fh[:] = False
    elif kind == "mixed":
        fh[:] = False
        for b, k in enumerate((0, 1, 3, 3, 6)):
            fh[b, :min(k + 1, int(nm[b].sum())), list(pr.CHANNELS)] = True
        fx[2, 0] = fx[4, 0] = False
    return nm, em, fx, fh, xk, hk, ctx


def kw_of(fx, fh):
    return dict(fixed_x_mask=dev(fx), fixed_h_mask=dev(fh))


# ----------------------------------------------------------------------------- 2. bit identities

@pytest.mark.parametrize("precision", BOTH)
@pytest.mark.parametrize("graph", [True, False], ids=["graph", "launches"])
def test_coinciding_and_empty_masks_give_the_whole_node_and_the_plain_bits(graph, precision):
    model, _, _ = make_model(32, T, precision=precision)
    model.use_graph = graph
    nm, em, fm, xk, hk, _ = make_case()
    B, N = nm.shape[:2]
    args = (dev(nm), dev(fm), dev(xk), dev(hk))
    whole = model.sample_inpaint(*args, sample_id_base=17, resamplings=2)
    fh1, fhF, empty = fm, fm.expand(B, N, 8).contiguous(), torch.zeros_like(fm)
    for kw in (dict(fixed_x_mask=dev(fm), fixed_h_mask=dev(fh1)), dict(fixed_h_mask=dev(fhF)), dict(fixed_x_mask=dev(fm))):
        got = model.sample_inpaint(*args, sample_id_base=17, resamplings=2, **kw)
        assert torch.equal(got[0], whole[0]) and torch.equal(got[1], whole[1])
    got = model.sample_inpaint(dev(nm), None, dev(xk), dev(hk), sample_id_base=17, resamplings=2, fixed_x_mask=dev(fm), fixed_h_mask=dev(fhF))
    assert torch.equal(got[0], whole[0]) and torch.equal(got[1], whole[1])
    # the few-step path and single steps
    w4 = model.sample_inpaint(*args, sample_id_base=17, steps=4)
    g4 = model.sample_inpaint(*args, sample_id_base=17, steps=4, fixed_x_mask=dev(fm), fixed_h_mask=dev(fhF))
    assert torch.equal(g4[0], w4[0]) and torch.equal(g4[1], w4[1])
    g = torch.Generator().manual_seed(2)
    z = orc.combined_noise(torch.randn(B, N, 3, generator=g), torch.randn(B, N, 8, generator=g), nm.float())
    ws = model.inpaint_steps(dev(z), 5, 3, *args, sample_id_base=4)
    gs = model.inpaint_steps(dev(z), 5, 3, *args, sample_id_base=4, fixed_x_mask=dev(fm), fixed_h_mask=dev(fhF))
    assert torch.equal(ws, gs)
    # empty masks: plain sampling
    plain = model.sample_from_masks(dev(nm), None, None, sample_id_base=17)
    got = model.sample_inpaint(dev(nm), None, dev(xk), dev(hk), sample_id_base=17, fixed_x_mask=dev(empty), fixed_h_mask=dev(empty))
    assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1])
    # and the whole-node call afterwards is untouched by the attachments before it
    again = model.sample_inpaint(*args, sample_id_base=17, resamplings=2)
    assert torch.equal(again[0], whole[0]) and torch.equal(again[1], whole[1])


# ----------------------------------------------------------------------------- 3. parity with the restatement over the oracle

@pytest.mark.parametrize("precision", BOTH)
@pytest.mark.parametrize("r", [1, 2])
def test_single_step_matches_the_restatement(lib, r, precision):
    s = 4
    model, sd, cfg = make_model(32, T, precision=precision)
    sd_np = fixture_model(load(FIXTURE[32]))[0]
    gg = gamma_grid_fp64(model, T)
    path = list(range(T, -1, -1))
    for kind in MASKS:
        nm, em, fx, fh, xk, hk, _ = parts_case(kind)
        B, N = nm.shape[:2]
        ids = [5 + b for b in range(B)]
        g = torch.Generator().manual_seed(1)
        z_t = orc.combined_noise(torch.randn(B, N, 3, generator=g), torch.randn(B, N, 8, generator=g), nm.float())
        net = er.RefNet(sd_np, cfg, T, nm, em, None)
        xh_known = torch.cat([xk, hk], dim=2)
        ref = pr.inpaint_parts_path_ref(lib, net, gg, path, T, z_t, nm, fx, fh, xh_known, r, SEED, ids, k_lo=T - s - 1, k_hi=T - s)[-1]
        for graph in (True, False):
            model.use_graph = graph
            got = model.inpaint_steps(dev(z_t), s + 1, s, dev(nm), None, dev(xk), dev(hk), resamplings=r, sample_id_base=5, **kw_of(fx, fh))
            rl, ma, bound = errors(got.cpu().numpy(), ref.numpy())
            print(f"parts single step {kind} r={r} [{precision}] graph={graph}: rel_l2 {rl:.2e} max_abs {ma:.2e} (bound {bound:.2e})")
            assert rl < REL_L2_TOL and ma < bound
            assert torch.all(got.cpu()[~nm.expand_as(got).bool()] == 0)


CHAINS = {"R1": dict(), "R2": dict(resamplings=2), "K4": dict(steps=4), "K4R2guided": dict(steps=4, resamplings=2, guidance_scale=2.0),
          "x0": dict(record="x0")}


@pytest.mark.parametrize("precision", BOTH)
@pytest.mark.parametrize("case", list(CHAINS))
def test_chain_matches_the_restatement(lib, case, precision):
    """Per state (the frames of keep_frames = K; record = "x0": the data prediction of every transition's last round) and for the
    returned (x, h): rel-L2 < 1e-4 and max-abs < 1e-4 max(1, |ref|) against the restatement over the oracle."""
    kw = dict(CHAINS[case])
    guided = "guidance_scale" in kw
    C_ = 1 if guided else 0
    model, sd, cfg = make_model(32, T, C_=C_, precision=precision)
    sd_np = fixture_model(load(FIXTURE[32]), context_node_nf=C_)[0]
    R, record = kw.get("resamplings", 1), kw.pop("record", "z")
    gg = gamma_grid_fp64(model, T)
    g32 = torch.as_tensor(gg, dtype=torch.float32).view(-1)
    path = paths.build_path(T, kw.get("steps"))
    K = len(path) - 1
    for kind in MASKS:
        nm, em, fx, fh, xk, hk, ctx = parts_case(kind, C_=C_)
        B, N = nm.shape[:2]
        ids = [9 + b for b in range(B)]
        net = er.RefNet(sd_np, cfg, T, nm, em, ctx)
        inner = gr.GuidedNet(net, er.RefNet(sd_np, cfg, T, nm, em, gr.null_ctx(nm)), 2.0, 0.0) if guided else net
        xh_known = torch.cat([xk, hk], dim=2)
        z = orc.combined_noise(*philox_raw(lib, SEED, ids, 0, N), nm.float())
        frames = []
        ref = pr.inpaint_parts_path_ref(lib, inner, gg, path, T, z, nm, fx, fh, xh_known, R, SEED, ids, x0_frames=frames)
        x, h, chain = model.sample_inpaint(dev(nm), None, dev(xk), dev(hk), context=dev(ctx), sample_id_base=9, keep_frames=K,
                                           record=record, **kw_of(fx, fh), **kw)
        assert torch.isfinite(chain).all()
        worst = 0.0
        for k in range(K - 1):                                # transition k arrives at position K - 1 - k, its frame at keep = K
            f = chain[K - 1 - k].cpu()
            if record == "z":
                rl, ma, bound = errors(f.numpy(), ref[k].numpy())
            else:
                zk, ek = frames[k]
                al, sg = float(torch.sqrt(torch.sigmoid(-g32[path[k]]))), float(torch.sqrt(torch.sigmoid(g32[path[k]])))
                rl, ma, bound = errors(f[:, :, :3].numpy(), (rr.x0_f32(zk, ek, al, sg, 1.0) * nm.float()).numpy())
            worst = max(worst, rl)
            print(f"parts chain {case} {kind} [{precision}] {'state' if record == 'z' else 'x0 frame'} {k + 1}/{K}: rel_l2 {rl:.2e} "
                  f"max_abs {ma:.2e} (bound {bound:.2e})")
            assert rl < REL_L2_TOL and ma < bound, (case, kind, precision, k)
        xr, hr = gr.decode_on_eps(net, ref[-1], inner.net(ref[-1], 0), philox_raw(lib, SEED, ids, T + 1, N), gg)
        xr, hr = pr.decode_fix_parts_ref(xr.float(), hr.float(), xk, hk, nm, fx, fh)
        ex, eh = errors(x.cpu().numpy(), xr.numpy()), errors(h.cpu().numpy(), hr.numpy())
        print(f"parts chain {case} {kind} [{precision}]: worst state {worst:.2e}; x rel_l2 {ex[0]:.2e} max_abs {ex[1]:.2e}; "
              f"h rel_l2 {eh[0]:.2e} max_abs {eh[1]:.2e}")
        assert ex[0] < REL_L2_TOL and ex[1] < ex[2] and eh[0] < REL_L2_TOL and eh[1] < eh[2]
        assert torch.equal(chain[0], torch.cat([x, h], dim=2))


# ----------------------------------------------------------------------------- 4. what comes back

@pytest.mark.parametrize("precision", BOTH)
def test_results_keep_the_known_parts_and_sample_the_rest(precision):
    model, _, _ = make_model(32, T, precision=precision)
    for kind in MASKS:
        nm, em, fx, fh, xk, hk, _ = parts_case(kind, seed=3)
        B, N = nm.shape[:2]
        x, h = model.sample_inpaint(dev(nm), None, dev(xk), dev(hk), resamplings=2, sample_id_base=9, **kw_of(fx, fh))
        x, h = x.cpu(), h.cpu()
        assert torch.isfinite(x).all() and torch.isfinite(h).all()
        assert torch.equal(h[fh], hk[fh])                                         # replaced channels: h_known exactly
        freeh = nm.expand_as(h) & ~fh
        assert not (h[freeh] == hk[freeh]).any()                                  # free parts are not the known values
        for b in range(B):
            f = fx[b, :, 0]
            if int(f.sum()) >= 1:
                d = (x - xk)[b][f]                                                # the Fx block: a pure translation of x_known
                mag = max(float(x[b][f].abs().max()), float(xk[b][f].abs().max()))
                assert float((d - d[0]).abs().max()) <= 2 * float(np.spacing(np.float32(mag))), (kind, b)
            fr_ = nm[b, :, 0] & ~f
            if int(fr_.sum()) >= 2:
                d = (x - xk)[b][fr_]
                assert float((d - d[0]).abs().max()) > 1e-3, (kind, b)            # free positions do not copy x_known
        assert torch.all(x[~nm.expand_as(x)] == 0) and torch.all(h[~nm.expand_as(h)] == 0)


def test_framed_call_uses_the_position_mask():
    """restraint_frame="known" with one obstacle and one 2 x 2 x 2 field: 'x_known_frame' on Fx is x_known to fp32 rounding, the
    energies are evaluated with the position mask, and a node with known features and a free position is pushed."""
    model, _, _ = make_model(32, T)
    nm, em, fx, fh, xk, hk, _ = parts_case("mixed", seed=4)
    xk = (xk + torch.tensor(fr.CENTRE) - torch.tensor([3.0, -2.0, 1.0])).contiguous()
    B, N = nm.shape[:2]
    c0 = xk[2, 1:3].mean(0)                                                      # molecule 2: Fx = nodes 1, 2; node 0 has known features only
    fld = Field(torch.arange(8.0).reshape(2, 2, 2), origin=(c0 - 4.0).tolist(), spacing=8.0, k=0.5, wall=0.1)
    rs = Restraints(obstacles=[[float(c0[0]), float(c0[1]), float(c0[2]), 6.0, 2.0]], fields=[fld])
    rkw = dict(restraints=rs, restraint_scale=0.05, restraint_clip=0.3, restraint_frame="known")
    call = lambda **k: model.sample_inpaint(dev(nm), None, dev(xk), dev(hk), sample_id_base=9, steps=4, **kw_of(fx, fh), **k)
    x, h, info = call(**rkw)
    plain = call()
    assert not torch.equal(x, plain[0])                                           # the restraints acted
    x, tau, xkf = x.cpu(), info["frame_shift"].cpu(), info["x_known_frame"].cpu()
    tol = 2.0 ** -23 * (x.abs().max() + xk.abs().max())
    assert ((xkf - xk).abs() * fx.float()).max() <= tol
    want_tau, tmag = fr.frame_shift_ref(x.numpy(), xk.numpy(), nm, fx)
    assert (np.abs(tau.numpy() - want_tau) <= 1e-12 * tmag).all() and (tau[0] == 0).all()      # molecule 0: |Fx| = 0
    want = rs.energy(x, nm, fixed_mask=fx, x_known=xk)
    assert torch.allclose(info["restraint_energy"].cpu(), want, rtol=1e-9, atol=1e-12)
    assert torch.allclose(info["restraint_field_energy"].cpu(), rs.field_energy(x, nm, fixed_mask=fx, x_known=xk), rtol=1e-9, atol=1e-12)
    assert torch.equal(h.cpu()[fh], hk[fh])
    # features known, nothing else: no frame, tau = 0 - the tables are read in the model's frame
    fx0 = torch.zeros_like(fx)
    _, _, info0 = model.sample_inpaint(dev(nm), None, dev(xk), dev(hk), sample_id_base=9, steps=4, **kw_of(fx0, fh), **rkw)
    assert (info0["frame_shift"].cpu() == 0).all()


def test_known_features_with_a_free_position_are_pushed():
    """hd_restrain_eps_framed with the position mask against the whole-node mask: the node that is fixed only in the latter moves
    with the block there (its own step is 0) and receives its own non-zero step under the position mask."""
    N, D, nv0 = 5, 11, 1.7
    nm = torch.ones(1, N, dtype=torch.bool)
    whole = torch.tensor([[True, True, True, False, False]])
    pos = torch.tensor([[False, True, True, False, False]])                     # node 0: known features, free position
    g = torch.Generator().manual_seed(11)
    z, eps, known = torch.randn(1, N, D, generator=g), torch.randn(1, N, D, generator=g), torch.randn(1, N, D, generator=g)
    known[:, :, :3] = (torch.tensor(fr.CENTRE) + torch.randn(1, N, 3, generator=g)) / nv0
    row = (0.8, 0.6, 0.75, float("inf"))
    x0 = rr.x0_f32(z, eps, row[0], row[1], nv0)
    bare = Bare(D, nm)
    try:
        out = {}
        for name, fm in (("pos", pos), ("whole", whole)):
            tau, _ = fr.frame_shift_ref(x0.numpy(), (known[:, :, :3] * nv0).numpy(), nm, fm)
            y = x0[0, 0].double().numpy() - tau[0] + 0.3                          # an obstacle on node 0, in the known frame
            rs = Restraints(obstacles=[[float(y[0]), float(y[1]), float(y[2]), 3.0, 2.0]])
            rs.attach(bare, torch.ones(1), nv0, torch.device(DEV), stream())
            zd, ed, kd, o, fd = dev(z).contiguous(), dev(eps).contiguous(), dev(known).contiguous(), torch.zeros(1, N, D, device=DEV), u8(fm)
            rc = bare.lib.hd_restrain_eps_framed(bare.h, bare.topo, zd.data_ptr(), ed.data_ptr(), (C.c_float * 4)(*row), fd.data_ptr(),
                                                 kd.data_ptr(), o.data_ptr(), stream())
            assert rc == 0, bare.lib.hd_last_error()
            out[name] = (o.cpu() - eps)[0, :, :3]
        step = out["pos"][0] - out["pos"][1]                                      # node 0 relative to the block
        print(f"restraint step of the feature-known node relative to the block: {step.tolist()} (whole-node mask: "
              f"{(out['whole'][0] - out['whole'][1]).tolist()})")
        assert float(step.abs().max()) > 1e-3
        assert float((out["whole"][0] - out["whole"][1]).abs().max()) <= 4 * 2.0 ** -23 * float(eps.abs().max() + out["whole"].abs().max())
    finally:
        bare.lib.hd_restraint_detach(bare.topo)
        bare.close()


# ----------------------------------------------------------------------------- 5. locality

def test_known_features_reach_the_free_positions_of_their_molecule_only():
    model, _, _ = make_model(32, T)
    nm, em, fx, fh, xk, hk, _ = parts_case("h_only", seed=5)
    B, N = nm.shape[:2]
    call = lambda hk_, lo=0, hi=B, **k: model.sample_inpaint(dev(nm[lo:hi]), None, dev(xk[lo:hi]), dev(hk_[lo:hi]), sample_id_base=30 + lo,
                                                             resamplings=2, **kw_of(fx[lo:hi], fh[lo:hi]), **k)
    x1, h1 = call(hk)
    hk2 = hk.clone()
    hk2[2, 1, 3] += 1.5                                                           # one known channel of molecule 2
    x2, h2 = call(hk2)
    assert not torch.equal(x1[2, :7], x2[2, :7])                                  # its (free) positions move
    for b in (0, 1, 3, 4):
        assert torch.equal(x1[b], x2[b]) and torch.equal(h1[b], h2[b])            # no bit of any other molecule
    # cutting the batch
    xa, ha = call(hk, 2, 4)
    assert torch.equal(xa, x1[2:4]) and torch.equal(ha, h1[2:4])
    # cutting the chain
    nm, em, fx, fh, xk, hk, _ = parts_case("mixed", seed=5)
    g = torch.Generator().manual_seed(6)
    z = dev(orc.combined_noise(torch.randn(B, N, 3, generator=g), torch.randn(B, N, 8, generator=g), nm.float()))
    steps = lambda zz, hi, lo: model.inpaint_steps(zz, hi, lo, dev(nm), None, dev(xk), dev(hk), resamplings=2, sample_id_base=3, **kw_of(fx, fh))
    assert torch.equal(steps(z, T, 0), steps(steps(steps(z, T, 5), 5, 2), 2, 0))


# ----------------------------------------------------------------------------- 6. graphs

def test_attaching_and_detaching_rebuild_once_and_other_masks_replay(lib):
    model, _, _ = make_model(32, T)
    nm, em, fm, xk, hk, _ = make_case()
    B, N = nm.shape[:2]
    nmd = dev(nm)
    args = (nmd, dev(fm), dev(xk), dev(hk))
    whole = model.sample_inpaint(*args, sample_id_base=2, steps=4)                # a topology that never had parts
    topo = model.dynamics.topology(nmd, None, B, N)
    builds = lambda: lib.hd_path_graph_builds(topo.ptr)
    n0 = builds()
    assert n0 >= 1
    _, _, fx, fh, _, _, _ = parts_case("mixed")
    a = model.sample_inpaint(nmd, None, dev(xk), dev(hk), sample_id_base=2, steps=4, **kw_of(fx, fh))
    assert builds() == n0 + 1                                                     # attaching builds once
    _, _, fx2, fh2, _, _, _ = parts_case("h_only")
    b = model.sample_inpaint(nmd, None, dev(xk), dev(hk), sample_id_base=2, steps=4, **kw_of(fx2, fh2))
    a2 = model.sample_inpaint(nmd, None, dev(xk), dev(hk), sample_id_base=2, steps=4, **kw_of(fx, fh))
    assert builds() == n0 + 1                                                     # other mask contents do not
    assert torch.equal(a[0], a2[0]) and torch.equal(a[1], a2[1]) and not torch.equal(a[0], b[0])
    again = model.sample_inpaint(*args, sample_id_base=2, steps=4)
    assert builds() == n0 + 2                                                     # detaching builds once ...
    assert torch.equal(again[0], whole[0]) and torch.equal(again[1], whole[1])    # ... and gives the bits of a fresh topology
    model.use_graph = False
    a3 = model.sample_inpaint(nmd, None, dev(xk), dev(hk), sample_id_base=2, steps=4, **kw_of(fx, fh))
    assert torch.equal(a[0], a3[0]) and torch.equal(a[1], a3[1]) and builds() == n0 + 2


# ----------------------------------------------------------------------------- 7. the command line

def test_cli_known_parts(tmp_path):
    from hierdiff_amd import sampler
    from hierdiff_amd.weights import synthetic_state_dict
    syn = synthetic_state_dict(9, 0, 32, 1, 2, True, 12, 1.0)
    ck = tmp_path / "diffusion.ckpt"
    torch.save({"state_dict": {"model." + k: torch.from_numpy(v.copy()) for k, v in syn.items()}}, ck)
    plain, known = tmp_path / "plain.pkl", tmp_path / "known.pkl"
    common = ["--checkpoint", str(ck), "--hidden-nf", "32", "--n-layers", "1", "--timesteps", "6"]
    assert sampler.main(common + ["--out", str(plain), "--batch-size", "8", "--num-batches", "1"]) == 0
    res = [m for m in pickle.load(open(plain, "rb"))[0] if m["x"].shape[0] >= 3][:4]
    assert len(res) == 4
    frag = [{"x": m["x"][:3].clone(), "h": m["h"][:3].clone()} for m in res]
    sampler.write_results(str(known), frag)
    out_h, out_x = tmp_path / "h.pkl", tmp_path / "x.pkl"
    assert sampler.main(common + ["--out", str(out_h), "--known", str(known), "--known-parts", "h", "--grow", "0", "--batch-size", "3"]) == 0
    laid, _ = pickle.load(open(out_h, "rb"))
    assert len(laid) == 4
    for m, f in zip(laid, frag):                              # the fragments laid out again: features kept, positions sampled
        assert tuple(m["x"].shape) == (3, 3) and torch.equal(m["h"], f["h"]) and torch.isfinite(m["x"]).all()
        d = m["x"] - f["x"]
        assert float((d - d[0]).abs().max()) > 1e-3
    assert sampler.main(common + ["--out", str(out_x), "--known", str(known), "--known-parts", "x", "--grow", "2", "--batch-size", "3"]) == 0
    grown, _ = pickle.load(open(out_x, "rb"))
    for m, f in zip(grown, frag):                             # positions kept as one block, features sampled, two fragments more
        assert tuple(m["x"].shape) == (5, 3) and tuple(m["h"].shape) == (5, 8) and torch.isfinite(m["h"]).all()
        d = m["x"][:3] - f["x"]
        mag = max(float(m["x"][:3].abs().max()), float(f["x"].abs().max()))
        assert float((d - d[0]).abs().max()) <= 2 * float(np.spacing(np.float32(mag)))
        assert not torch.equal(m["h"][:3], f["h"])
