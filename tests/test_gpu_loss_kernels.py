"""The fused training loss (`hd_vlb_loss_forward` / `_backward`, `hd_vlb_zt`; csrc/k_loss.hpp) and the one-launch helpers
`hd_edge_prep` and `hd_linear`, called at the C ABI and compared with float64: the restatement of tests/loss_reference.py and its
autograd gradients for the loss, torch slicing for the layout kernel, a float64 product for the dense layer.  Shapes: more than one
trip of the kernels' 256-thread loops, partly filled waves, ragged molecules; inputs: the integer-feature likelihood where its
derivatives do not vanish (zone A) and where it saturates (zone C), a non-zero volume term, a non-constant incoming gradient.

The band 1e-10 < bracket < 1e-3 of the integer likelihood is left out (tests/loss_reference.py says why), and g_t - g_s stays above
0.02: below it the reference's `exp(g_t - g_s) - 1` in fp32 loses more than the 1e-5 value bar - known properties of the expressions
the kernel keeps for parity with the reference, recorded here and not changed.

Every test prints its worst measured error over its bar next to the same figure of the restatement run in fp32 on the CPU."""
import ctypes as C

import pytest
import torch

from hierdiff_amd import _lib
from tests import loss_reference as lr
from tests.test_gpu_parity import DEV

pytestmark = pytest.mark.gpu

GUARD = 64                      # floats behind every output buffer
SENT = -12345.5                 # what they must still hold afterwards


def _lib_and_stream():
    return _lib.load(), torch.cuda.current_stream(DEV).cuda_stream


def _guarded(n, fill=SENT):
    return torch.full((n + GUARD,), fill, device=DEV, dtype=torch.float32)


def _guard_intact(buf, n):
    return bool((buf[n:] == SENT).all())


def _ids(v):
    return "-".join(f"{x:g}" for x in v)


# ----------------------------------------------------------------------------- hd_vlb_loss_forward / hd_vlb_loss_backward

@pytest.mark.parametrize("variant", lr.VLB_VARIANTS, ids=_ids)
@pytest.mark.parametrize("shape", lr.VLB_SHAPES, ids=_ids)
def test_vlb_loss_matches_the_float64_restatement(shape, variant):
    """loss, err, dnet, dzt and dgam [4][B] of one launch per direction against the float64 restatement and its autograd, on the
    designed inputs (the CPU tier checks their conditioning).  Bars: loss within 1e-5 (|K| + est |L| + |C0| + |delta|), err 1e-5
    relative, dnet / dzt rel-L2 < 1e-4, dgam element by element within 1e-4 of the float64 sum of its absolute terms.  Exact zeros
    where the loss does not depend on an input, guard floats behind every output, same bits on a second call."""
    lib, st = _lib_and_stream()
    B, N, D, int_nf, cont_nf = shape
    l2, nv2, nb2, log_nv0 = variant
    inp = lr.vlb_case_inputs(shape, variant)
    ref, scales, cpu32 = lr.vlb_expected(shape, variant)
    d = {k: v.to(DEV).contiguous() for k, v in inp.items()}
    sizes = dict(loss=B, err=B, dnet=B * N * D, dzt=B * N * D, dgam=4 * B)

    def run():
        o = {k: _guarded(n) for k, n in sizes.items()}
        head = (0, B, N, D, int_nf, cont_nf, int(l2), lr.T_STEPS, nv2, nb2, log_nv0, d["net"].data_ptr(), d["zt"].data_ptr(),
                d["xh"].data_ptr(), d["eps"].data_ptr(), d["nm"].data_ptr(), d["gam"].data_ptr(), d["t_int"].data_ptr())
        _lib.check(lib.hd_vlb_loss_forward(*head, o["loss"].data_ptr(), o["err"].data_ptr(), st), "hd_vlb_loss_forward")
        _lib.check(lib.hd_vlb_loss_backward(*head, d["gout"].data_ptr(), o["dnet"].data_ptr(), o["dzt"].data_ptr(),
                                            o["dgam"].data_ptr(), st), "hd_vlb_loss_backward")
        torch.cuda.synchronize()
        return o

    first, second = run(), run()
    for k, n in sizes.items():
        assert _guard_intact(first[k], n), f"{k}: written past its end"
        assert torch.equal(first[k], second[k]), f"{k}: a second call gives other bits"
        assert torch.isfinite(first[k][:n]).all(), k
    got = dict(loss=first["loss"][:B], err=first["err"][:B], dnet=first["dnet"][:B * N * D].view(B, N, D),
               dzt=first["dzt"][:B * N * D].view(B, N, D), dgam=first["dgam"][:4 * B].view(4, B))
    got = {k: v.cpu().double() for k, v in got.items()}
    ratios = lr.vlb_ratios(got, ref, scales)
    print(f"k_vlb {shape} l2={l2} nv2={nv2:g} nb2={nb2:g} log_nv0={log_nv0:.3f}: error / bar, kernel (fp32 restatement on the CPU): "
          + ", ".join(f"{k} {v:.2e} ({cpu32[k]:.2e})" for k, v in ratios.items()))
    # where the loss does not depend on an input the gradient is exactly 0
    t0 = inp["t_int"] == 0
    off_int = torch.ones(D, dtype=torch.bool)
    off_int[3:3 + int_nf] = False
    assert float(got["dzt"][:, :, off_int].abs().max()) == 0.0, "dzt off the integer columns"
    if bool((~t0).any()):
        assert float(got["dzt"][~t0].abs().max()) == 0.0, "dzt on t > 0 rows"
    assert float(got["dnet"][t0][:, :, 3:].abs().max()) == 0.0, "dnet on the feature columns of t = 0 rows"
    for k, v in ratios.items():
        assert v < 1.0, (k, v)


# ----------------------------------------------------------------------------- hd_vlb_zt

@pytest.mark.parametrize("ND", lr.ZT_SIZES)
def test_vlb_zt_both_directions_match_float64(ND):
    """z_t = alpha(g_t) xh + sigma(g_t) eps and d/dg_t of it against a random dzt, g_t from -30 to 30 (one per molecule), ND below,
    at and above one trip of the loop: forward rel-L2 < 1e-5 per molecule, dgt within 1e-4 of the float64 sum of its absolute terms."""
    lib, st = _lib_and_stream()
    inp = lr.zt_inputs(ND)
    B = inp["xh"].shape[0]
    zt64, dgt64, scale = lr.zt_evaluate(inp, torch.float64)
    zt32, dgt32, _ = lr.zt_evaluate(inp, torch.float32)
    d = {k: v.to(DEV).contiguous() for k, v in inp.items()}
    outs = []
    for _ in range(2):
        zt, dgt = _guarded(B * ND), _guarded(B)
        _lib.check(lib.hd_vlb_zt(0, B, ND, d["xh"].data_ptr(), d["eps"].data_ptr(), d["gt"].data_ptr(), zt.data_ptr(), None, None, st),
                   "hd_vlb_zt")
        _lib.check(lib.hd_vlb_zt(0, B, ND, d["xh"].data_ptr(), d["eps"].data_ptr(), d["gt"].data_ptr(), None, d["dzt"].data_ptr(),
                                 dgt.data_ptr(), st), "hd_vlb_zt")
        torch.cuda.synchronize()
        outs.append((zt, dgt))
    (zt, dgt), (zt2, dgt2) = outs
    assert _guard_intact(zt, B * ND) and _guard_intact(dgt, B)
    assert torch.equal(zt, zt2) and torch.equal(dgt, dgt2)
    got_zt, got_dgt = zt[:B * ND].view(B, ND).cpu().double(), dgt[:B].cpu().double()
    fwd = max(lr.rel_l2_t(got_zt[b], zt64[b]) for b in range(B)) / lr.VALUE_TOL
    fwd32 = max(lr.rel_l2_t(zt32[b], zt64[b]) for b in range(B)) / lr.VALUE_TOL
    bwd = float(((got_dgt - dgt64).abs() / (lr.GRAD_TOL * scale)).max())
    bwd32 = float(((dgt32 - dgt64).abs() / (lr.GRAD_TOL * scale)).max())
    print(f"k_vlb_zt ND={ND}: error / bar, kernel (fp32 restatement on the CPU): zt {fwd:.2e} ({fwd32:.2e}), dgt {bwd:.2e} ({bwd32:.2e})")
    assert lr.rel_l2_t(got_zt, zt64) < lr.VALUE_TOL and fwd < 1.0
    assert bwd < 1.0


# ----------------------------------------------------------------------------- hd_edge_prep

@pytest.mark.parametrize("H", [1, 3, 32, 64, 128, 256])
def test_edge_prep_is_a_bit_exact_copy_both_ways(H):
    """dir 0: W1 [H][2H + 2], b1 -> Wst [2H][H] = [W1[:, :H] ; W1[:, H:2H]], bst = [b1 | 0], wrd [2][H] = the two distance columns,
    bit for bit.  dir 1: dWst, dwrd -> every element of dW1, with b1 = bst = NULL.  dir 0 then dir 1 is the identity."""
    lib, st = _lib_and_stream()
    g = torch.Generator().manual_seed(H)
    W1 = torch.randn(H, 2 * H + 2, generator=g).to(DEV)
    b1 = torch.randn(H, generator=g).to(DEV)
    Wst, bst, wrd = _guarded(2 * H * H), _guarded(2 * H), _guarded(2 * H)
    before = W1.clone()
    _lib.check(lib.hd_edge_prep(0, H, 0, W1.data_ptr(), b1.data_ptr(), Wst.data_ptr(), bst.data_ptr(), wrd.data_ptr(), st), "hd_edge_prep")
    torch.cuda.synchronize()
    assert _guard_intact(Wst, 2 * H * H) and _guard_intact(bst, 2 * H) and _guard_intact(wrd, 2 * H)
    assert torch.equal(W1, before)
    assert torch.equal(Wst[:2 * H * H].view(2 * H, H), torch.cat([W1[:, :H], W1[:, H:2 * H]], 0))
    assert torch.equal(bst[:2 * H], torch.cat([b1, torch.zeros(H, device=DEV)]))
    assert torch.equal(wrd[:2 * H].view(2, H)[0], W1[:, 2 * H]) and torch.equal(wrd[:2 * H].view(2, H)[1], W1[:, 2 * H + 1])
    # the way back from random gradients into a NaN-filled dW1: every element written
    dWst = torch.randn(2 * H, H, generator=g).to(DEV)
    dwrd = torch.randn(2, H, generator=g).to(DEV)
    n = H * (2 * H + 2)
    dW1 = _guarded(n)
    dW1[:n] = float("nan")
    _lib.check(lib.hd_edge_prep(0, H, 1, dW1.data_ptr(), None, dWst.data_ptr(), None, dwrd.data_ptr(), st), "hd_edge_prep")
    torch.cuda.synchronize()
    assert _guard_intact(dW1, n)
    assert torch.equal(dW1[:n].view(H, 2 * H + 2), torch.cat([dWst[:H], dWst[H:], dwrd.t()], 1))
    # round trip
    back = _guarded(n)
    back[:n] = float("nan")
    _lib.check(lib.hd_edge_prep(0, H, 1, back.data_ptr(), None, Wst.data_ptr(), None, wrd.data_ptr(), st), "hd_edge_prep")
    torch.cuda.synchronize()
    assert _guard_intact(back, n) and torch.equal(back[:n].view(H, 2 * H + 2), W1)


# ----------------------------------------------------------------------------- hd_linear

def _linear_call(lib, st, x_ptr, M, K, ldx, W_ptr, b_ptr, N, act, ldy):
    """One hd_linear call into a sentinel-filled y [M][ldy] with guard floats behind it; returns the whole buffer."""
    y = _guarded(M * ldy)
    _lib.check(lib.hd_linear(0, x_ptr, M, K, ldx, W_ptr, b_ptr, N, act, y.data_ptr(), ldy, st), "hd_linear")
    return y


@pytest.mark.parametrize("M,K,N", lr.LINEAR_SHAPES)
def test_linear_matches_float64_with_padding_activations_and_saturation(M, K, N):
    """y = act(x W^T + b) for every combination of ldx in {K, K + 1, K + 4} (NaN in the padding columns of x), ldy in {N, N + 3}
    (sentinel kept in the padding columns of y), act in {none, SiLU, sigmoid}, bias given / NULL: rel-L2 < 1e-5 against float64,
    pre-activations out to +-100 finite and right in saturation.  The float4 and the scalar k-loop are one fmaf chain in one order: every
    ldx gives the same bits."""
    lib, st = _lib_and_stream()
    x, W, b = lr.linear_inputs(M, K, N)
    Wd, bd = W.to(DEV), b.to(DEV)
    refs = {(act, bias): lr.linear_ref(x.double(), W.double(), b.double() if bias else None, act) for act in (0, 1, 2) for bias in (True, False)}
    cpu32 = {(act, bias): lr.linear_ref(x, W, b if bias else None, act).double() for act, bias in refs}
    if M * N >= 100:
        assert float(refs[0, True].max()) > 100 and float(refs[0, True].min()) < -100
    worst = worst32 = 0.0
    bits = {}
    for ldx in (K, K + 1, K + 4):
        xp = torch.full((M, ldx), float("nan"), device=DEV)
        xp[:, :K] = x.to(DEV)
        for ldy in (N, N + 3):
            for act in (0, 1, 2):
                for bias in (True, False):
                    y = _linear_call(lib, st, xp.data_ptr(), M, K, ldx, Wd.data_ptr(), bd.data_ptr() if bias else None, N, act, ldy)
                    torch.cuda.synchronize()
                    assert _guard_intact(y, M * ldy)
                    y2 = y[:M * ldy].view(M, ldy)
                    assert bool((y2[:, N:] == SENT).all()), "padding columns of y written"
                    got = y2[:, :N].cpu()
                    assert torch.isfinite(got).all()
                    ref = refs[act, bias]
                    worst = max(worst, lr.rel_l2_t(got.double(), ref) / lr.VALUE_TOL)
                    worst32 = max(worst32, lr.rel_l2_t(cpu32[act, bias], ref) / lr.VALUE_TOL)
                    assert lr.rel_l2_t(got.double(), ref) < lr.VALUE_TOL, (ldx, ldy, act, bias)
                    # saturation: sigmoid(-40) = 4e-18, and 1 - sigmoid(40) is below half an ulp of 1
                    lo, hi = refs[0, bias] < -40, refs[0, bias] > 40
                    if act == 2:
                        assert bool((got[lo] >= 0).all()) and bool((got[lo] <= 1e-15).all()) and bool((got[hi] == 1).all())
                    if act == 1:
                        assert bool((got[lo].abs() <= 1e-12).all())
                    key = (ldy, act, bias)
                    assert torch.equal(bits.setdefault(key, got), got), f"ldx = {ldx} gives other bits than ldx = {K}"
    print(f"k_linear M={M} K={K} N={N}: worst rel-L2 / bar over 36 calls, kernel {worst:.2e} (torch fp32 on the CPU {worst32:.2e})")


def test_linear_with_no_rows_writes_nothing():
    lib, st = _lib_and_stream()
    x, W, y = torch.zeros(8, device=DEV), torch.zeros(8, device=DEV), _guarded(0)
    assert lib.hd_linear(0, x.data_ptr(), 0, 8, 8, W.data_ptr(), None, 1, 0, y.data_ptr(), 1, st) == 0
    torch.cuda.synchronize()
    assert _guard_intact(y, 0)


def test_linear_through_a_misaligned_view_gives_the_aligned_bits():
    """K = 8 and ldx = 8 take the float4 loop only when x and W are 16-byte aligned: the same values one float further into a
    buffer take the scalar loop and give the same bits."""
    lib, st = _lib_and_stream()
    M, K, N = 257, 8, 49
    x, W, b = lr.linear_inputs(M, K, N)
    xd, Wd, bd = x.to(DEV), W.to(DEV), b.to(DEV)
    xo, Wo = torch.zeros(M * K + 4, device=DEV), torch.zeros(N * K + 4, device=DEV)
    xo[1:1 + M * K] = xd.reshape(-1)
    Wo[1:1 + N * K] = Wd.reshape(-1)
    assert xd.data_ptr() % 16 == 0 and Wd.data_ptr() % 16 == 0 and xo.data_ptr() % 16 == 0 and Wo.data_ptr() % 16 == 0
    for act in (0, 1):
        want = _linear_call(lib, st, xd.data_ptr(), M, K, K, Wd.data_ptr(), bd.data_ptr(), N, act, N)
        for xp, wp in ((xo.data_ptr() + 4, Wd.data_ptr()), (xd.data_ptr(), Wo.data_ptr() + 4), (xo.data_ptr() + 4, Wo.data_ptr() + 4)):
            got = _linear_call(lib, st, xp, M, K, K, wp, bd.data_ptr(), N, act, N)
            torch.cuda.synchronize()
            assert torch.equal(got, want)
    ref = lr.linear_ref(x.double(), W.double(), b.double(), 1)
    assert lr.rel_l2_t(want[:M * N].view(M, N).cpu().double(), ref) < lr.VALUE_TOL


# ----------------------------------------------------------------------------- documented refusals

def test_bad_arguments_are_refused_on_the_host():
    """Every argument check of the five entry points returns < 0 and names its function in hd_last_error().  Each call below fails one
    check, so none of them reaches a launch; the shapes are ones the buffer would hold all the same."""
    lib, st = _lib_and_stream()
    p = torch.zeros(64, device=DEV).data_ptr()
    nodev = lib.hd_device_count()

    def refused(name, rc):
        assert rc < 0, name
        assert name.encode() in lib.hd_last_error(), (name, lib.hd_last_error())

    # hd_vlb_loss_forward / _backward: (device, B, N, D, int_nf, cont_nf) then the tensors
    good = dict(device=0, B=1, N=1, D=4, int_nf=1, cont_nf=0)
    bad_shapes = [dict(B=0), dict(N=0), dict(D=3), dict(int_nf=-1), dict(cont_nf=-1), dict(int_nf=1, cont_nf=1), dict(device=nodev),
                  dict(device=-1)]
    for name, n_ptr in (("hd_vlb_loss_forward", 9), ("hd_vlb_loss_backward", 11)):
        fn = getattr(lib, name)
        for change in bad_shapes:
            a = {**good, **change}
            refused(name, fn(a["device"], a["B"], a["N"], a["D"], a["int_nf"], a["cont_nf"], 0, 10.0, 1.0, 0.0, 0.0, *([p] * n_ptr), st))
        for i in range(n_ptr):
            ptrs = [p] * n_ptr
            ptrs[i] = None
            refused(name, fn(0, 1, 1, 4, 1, 0, 0, 10.0, 1.0, 0.0, 0.0, *ptrs, st))
    # hd_vlb_zt (device, B, ND, xh, eps, gt, zt, dzt, dgt)
    for args in ((0, 0, 4, p, p, p, p, None, None), (0, 1, 0, p, p, p, p, None, None), (0, 1, 4, None, p, p, p, None, None),
                 (0, 1, 4, p, None, p, p, None, None), (0, 1, 4, p, p, None, p, None, None), (0, 1, 4, p, p, p, None, None, None),
                 (0, 1, 4, p, p, p, None, p, None), (nodev, 1, 4, p, p, p, p, None, None), (-1, 1, 4, p, p, p, p, None, None)):
        refused("hd_vlb_zt", lib.hd_vlb_zt(*args, st))
    # hd_edge_prep (device, H, dir, W1, b1, Wst, bst, wrd)
    for args in ((0, 0, 0, p, p, p, p, p), (0, 1, 0, None, p, p, p, p), (0, 1, 0, p, p, None, p, p), (0, 1, 0, p, p, p, p, None),
                 (0, 1, 0, p, None, p, p, p), (0, 1, 0, p, p, p, None, p), (0, 1, 1, None, None, p, None, p), (nodev, 1, 0, p, p, p, p, p),
                 (-1, 1, 1, p, None, p, None, p)):
        refused("hd_edge_prep", lib.hd_edge_prep(*args, st))
    # hd_linear (device, x, M, K, ldx, W, b, N, act, y, ldy)
    for args in ((0, None, 1, 1, 1, p, p, 1, 0, p, 1), (0, p, 1, 1, 1, None, p, 1, 0, p, 1), (0, p, 1, 1, 1, p, p, 1, 0, None, 1),
                 (0, p, -1, 1, 1, p, p, 1, 0, p, 1), (0, p, 1, 0, 1, p, p, 1, 0, p, 1), (0, p, 1, 1, 1, p, p, 0, 0, p, 1),
                 (0, p, 1, 2, 1, p, p, 1, 0, p, 1), (0, p, 1, 1, 1, p, p, 2, 0, p, 1), (0, p, 1, 1, 1, p, p, 1, -1, p, 1),
                 (0, p, 1, 1, 1, p, p, 1, 3, p, 1), (nodev, p, 1, 1, 1, p, p, 1, 0, p, 1), (-1, p, 1, 1, 1, p, p, 1, 0, p, 1)):
        refused("hd_linear", lib.hd_linear(*args, st))
