"""GPU tier: the edge layer on its own - hd_edge_layer_forward[_s] / hd_edge_layer_backward[_s] through the C ABI against the
float64 restatement of one edge layer (tests/edge_layer_reference.py), tensor by tensor and row by row.

Bars (tests/edge_layer_reference.py, EXPERIMENTS.md section AO): per family of tensors the kernels' per-row error
against float64 is at most `margin x the error of the float32 CPU evaluation of the same graph on the same case`, and beside it
the suite's outer bar, rel-L2 < 1e-4 per tensor (tests/helpers.py).

Batches (those of tests/test_gpu_edge_chunk_peel.py; tile counts asserted on a 256-CU device, so that a changed launch rule does
not quietly test another kernel):
  SMALL  [5, 17, 30]          37 tiles     width >= 128: k_edge_split; no kept pre2 there (hd_edge_layer_save_rows == 0)
  WHOLE  SMALL + 27 x [30]    773 tiles    width >= 128: plain k_edge (the packed form at 256)
  MIXED  SMALL + 37 x [30]    1,045 tiles  width >= 128: k_edge_mixed
  WIDE   [70, 40, 3, 1], N = 70, a general mask with one self edge and one asymmetric hole: nodes with 138 and 78 incident edges
         (k_edge_dx: three and two rounds of 64), a node without edges
Every output and workspace is filled with NaN before a call: the kernels write every row (of escal the columns the layer
defines: 4:6 always, 0:4 in coordinate layers; 6:8 are the record's spare floats).
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import egnn_oracle as orc
from tests import edge_layer_reference as elr
from tests.helpers import assert_parity
from tests.test_gpu_parity import DEV, build_dynamics

pytestmark = pytest.mark.gpu

N_CU = 256
HEAD = [5, 17, 30]
BATCHES = {"small": (HEAD, 30), "whole": (HEAD + [30] * 27, 30), "mixed": (HEAD + [30] * 37, 30), "wide": ([70, 40, 3, 1], 70)}
TILES = {"small": 37, "whole": 773, "mixed": 1045}
CASES = [(b, H) for b in ("small", "wide") for H in (32, 64, 128, 256)] + [(b, H) for b in ("whole", "mixed") for H in (128, 256)]
KEPT = [(b, H) for b in ("whole", "mixed") for H in (128, 256)] + [("small", 32), ("small", 64)]
ODD = [(b, H) for b in ("small", "wide") for H in (64, 256)]
# variant -> (handle options, options of the restatement)
VARIANTS = {
    "plain": ({}, {}),                                                       # norm_constant = 0 (the self edge of WIDE: radial = 0)
    "x0far": ({}, {}),                                                       # x0 = 3 x + shift
    "saturate": ({}, {}),                                                    # |pre1| reaches 60 on a tenth of the rows
    "nc1": (dict(norm_constant=1.0), dict(norm_constant=1.0)),
    "noba": ({}, {}),                                                        # attention on, ba = NULL
    "plainhead": (dict(attention=False, tanh=False), dict(attention=False, tanh=False)),
    "mean": (dict(aggregation_method="mean"), {}),
}
RATIOS = {}       # (family, batch, H) -> worst err(kernel) / err(float32 CPU) seen in this process (the table of EXPERIMENTS.md)


# ----------------------------------------------------------------------------- cases, references (once per process)
@functools.lru_cache(maxsize=None)
def masks(batch):
    n_list, N = BATCHES[batch]
    nm, em = orc.canonical_masks(n_list, N)
    if batch == "wide":
        em = em.clone()
        em[1, 5, 5] = True          # a self edge
        em[0, 0, 1] = False         # an asymmetric hole
    return nm, em


@functools.lru_cache(maxsize=None)
def table(batch):
    nm, em = masks(batch)
    return elr.layout(nm.numpy()[..., 0], em.numpy())


def _f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def inputs(batch, H, variant):
    tab = table(batch)
    inp = elr.draw_inputs(tab["M"], H, 1000 + H + len(BATCHES[batch][0]))
    if variant == "noba":
        inp["ba"] = np.zeros(1)     # what the restatement sees; the device gets a NULL pointer
    if variant == "x0far":
        inp["x0"] = _f32(3.0 * inp["x"] + np.array([4.0, -2.0, 1.0, 0.0]))
    if variant == "saturate":
        AB = inp["AB"].copy()
        AB[::10, :H] *= 60.0 / np.abs(AB[::10, :H]).max(1, keepdims=True)       # every tenth receiving node: |A_i| reaches 60
        inp["AB"] = _f32(AB)
    return inp


@functools.lru_cache(maxsize=None)
def gouts(batch, H, coord):
    """A random gradient, and one that is non-zero on the second molecule only."""
    tab = table(batch)
    g = _f32(np.random.default_rng(7 + H).standard_normal((tab["M"], 4 if coord else H)))
    one = g * (tab["node_of"] // tab["N"] == 1)[:, None]
    return g, one


def options(batch, variant):
    o = elr.Opts(**VARIANTS[variant][1])
    if variant == "mean":
        o.norm = float(BATCHES[batch][1])
    return o


@functools.lru_cache(maxsize=None)
def reference(batch, H, coord, variant="plain"):
    """float64 results and, per tensor, the float32 CPU evaluation's error against them."""
    tab, inp, opts = table(batch), inputs(batch, H, variant), options(batch, variant)
    gs = gouts(batch, H, coord)
    r64 = elr.edge_layer(inp, tab, opts, coord, gs)
    r32 = elr.edge_layer(inp, tab, opts, coord, gs, float32=True)
    e32 = {"out": elr.err(r32["out"], r64["out"]), "P": elr.err(r32["P"], r64["P"]),
           "bwd": [{k: elr.err(b32[k], b64[k]) for k in b64 if not k.endswith("_rows")} for b32, b64 in zip(r32["bwd"], r64["bwd"])]}
    for b in r64["bwd"]:
        for k in [k for k in b if k.endswith("_rows")]:
            del b[k]
    return r64, e32


@functools.lru_cache(maxsize=None)
def handle(H, variant="plain", precision="fp32"):
    from hierdiff_amd.weights import synthetic_state_dict
    kw = VARIANTS[variant][0]
    sd_np = synthetic_state_dict(9, 0, H, 1, 2, kw.get("attention", True), 900 + H, 1.0)
    dyn = build_dynamics(sd_np, H, 1, **kw)
    dyn.precision = precision
    return dyn


def topology(dyn, batch):
    nm, em = masks(batch)
    B, N = nm.shape[:2]
    nmd, emd = _device_masks(batch)
    topo = dyn.topology(nmd, emd, B, N)
    info, tab = topo.info(), table(batch)
    if batch in TILES:
        assert info["tiles"] == TILES[batch]
        assert torch.cuda.get_device_properties(DEV).multi_processor_count == N_CU
    n_wg = (info["tiles"] + 3) // 4
    assert info["nodes"] == tab["M"] and max(1, 4 * n_wg) == tab["tiles"] and 32 * tab["tiles"] == tab["rows"]
    return topo


@functools.lru_cache(maxsize=None)
def _device_masks(batch):
    nm, em = masks(batch)
    return nm.contiguous().to(DEV), em.contiguous().to(DEV)


# ----------------------------------------------------------------------------- calls
def _lib():
    from hierdiff_amd import _lib as L
    return L, L.load()


def device_inputs(inp):
    t = lambda a: None if a is None else torch.tensor(np.asarray(a), dtype=torch.float32, device=DEV).contiguous()
    return {k: t(inp[k]) for k in ("AB", "x", "x0", "wrd", "W2", "b2", "wa", "ba")}


def _p(t):
    return None if t is None else t.data_ptr()


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV, dtype=torch.float32)


def save_rows(dyn, topo, prec=0):
    return int(_lib()[1].hd_edge_layer_save_rows(dyn._handle(), topo.ptr, prec))


def forward(dyn, topo, tab, coord, d, prec=0, keep=False):
    """out [M, H or 4] (and the kept pre2) of hd_edge_layer_forward / _forward_s; everything NaN before the call."""
    L, lib = _lib()
    H = d["b2"].shape[0]
    out = _nan(max(1, tab["M"]), 4 if coord else H)
    args = [_p(d[k]) for k in ("AB", "x", "x0", "wrd", "W2", "b2", "wa", "ba")]
    if not keep and prec == 0:
        L.check(lib.hd_edge_layer_forward(dyn._handle(), topo.ptr, int(coord), *args, _p(out), None), "hd_edge_layer_forward")
        return out, None
    pre2 = _nan(save_rows(dyn, topo, prec), H) if keep else None
    L.check(lib.hd_edge_layer_forward_s(dyn._handle(), topo.ptr, int(coord), prec, *args, _p(out), _p(pre2), None),
            "hd_edge_layer_forward_s")
    return out, pre2


WS = ("G2", "P", "G1", "escal", "colpart", "bapart", "b2part", "wrdpart", "dAB", "dx", "dx0")


def backward(dyn, topo, tab, coord, d, gout, prec=0, pre2=None, want_rc=False):
    """Every output and workspace of hd_edge_layer_backward / _backward_s, sized as hierdiff_amd/training.py::_TrainTables sizes
    them (tiles = max(1, 4 n_wg), rows = 32 tiles) and NaN before the call."""
    L, lib = _lib()
    H, M, rows, tiles = d["b2"].shape[0], max(1, tab["M"]), tab["rows"], tab["tiles"]
    o = dict(G2=_nan(rows, H), P=_nan(rows, H), G1=_nan(rows, H), escal=_nan(rows, 8), colpart=_nan(tiles, H), bapart=_nan(tiles),
             b2part=_nan(tiles, H), wrdpart=_nan(tiles, 2, H), dAB=_nan(M, 2 * H), dx=_nan(M, 4), dx0=_nan(M, 4))
    g = torch.tensor(np.asarray(gout), dtype=torch.float32, device=DEV).contiguous()
    args = [_p(d[k]) for k in ("AB", "x", "x0", "wrd", "W2", "b2", "wa", "ba")]
    outs = [_p(o[k]) for k in WS]
    f16ws = None
    if prec == 3 and pre2 is not None:
        nw = C.c_int(0)
        f16ws = _nan(int(lib.hd_edge_layer_f16ws_floats(dyn._handle(), topo.ptr, C.byref(nw))))
        o["f16ws"], o["n_wg"] = f16ws, nw.value
    if prec == 0 and pre2 is None:
        rc = lib.hd_edge_layer_backward(dyn._handle(), topo.ptr, int(coord), *args, _p(g), *outs, None)
    else:
        rc = lib.hd_edge_layer_backward_s(dyn._handle(), topo.ptr, int(coord), prec, *args, _p(g), _p(pre2), _p(f16ws), *outs, None)
    if want_rc:
        return rc
    L.check(rc, "hd_edge_layer_backward")
    torch.cuda.synchronize()
    return o


def defined(o, coord):
    """The tensors of a backward call the contract defines: escal by its column groups."""
    t = {k: o[k] for k in WS if k != "escal"}
    t["escal_rd"] = o["escal"][:, 4:6]
    if coord:
        t["escal_u"], t["escal_phi"] = o["escal"][:, 0:3], o["escal"][:, 3:4]
    return t


def assert_same_bits(a, b, coord, what):
    ta, tb = defined(a, coord), defined(b, coord)
    for k in ta:
        assert torch.equal(ta[k], tb[k]), f"{what}: {k} differs, max {(ta[k] - tb[k]).abs().max().item():.3e}"


class Checker:
    """Collects every tensor of a test that misses its bar (one failing row should not hide the next tensor's)."""

    def __init__(self, batch, H, what):
        self.batch, self.H, self.what, self.failed = batch, H, what, []

    def __call__(self, name, got, ref64, e32, family=None):
        fam = family or elr.FAMILY[name]
        got = got.detach().double().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, dtype=np.float64)
        e = elr.err(got, ref64)
        yard = max(e32, elr.YARDSTICK_FLOOR)
        key = (fam, self.batch, self.H)
        RATIOS[key] = max(RATIOS.get(key, 0.0), e / yard)
        print(f"{self.what} {name}: err {e:.3e}  float32 CPU {e32:.3e}  ratio {e / yard:.2f}  (margin {elr.MARGINS[fam]:g})")
        if not e <= elr.bar(fam, e32):
            self.failed.append(f"{name}: err {e:.3e} > {elr.MARGINS[fam]:g} x {yard:.3e}")
        try:
            assert_parity(got, np.asarray(ref64).reshape(got.shape), f"{self.what} {name}")
        except AssertionError as ex:
            self.failed.append(str(ex))

    def done(self):
        assert not self.failed, f"{self.what}:\n  " + "\n  ".join(self.failed)


def check_backward(ck, o, b64, e32, tab, coord, with_ba, family=None, names=None):
    """A backward call's results against the restatement: per-edge and per-node tensors as they are, the per-tile partials
    and G2^T P summed in float64 on the host."""
    t = defined(o, coord)
    for k, v in t.items():
        assert not torch.isnan(v).any(), f"{ck.what}: {k} has rows the call left unwritten"
    got = {k: t[k] for k in ("G2", "P", "G1", "escal_rd", "dAB", "dx", "dx0") + (("escal_u", "escal_phi") if coord else ())}
    f64 = lambda v: v.double().cpu()
    got["db2"] = f64(o["b2part"]).sum(0)[None]
    got["dwa"] = f64(o["colpart"]).sum(0)[None]
    got["dwrd"] = f64(o["wrdpart"]).sum(0)
    got["dW2"] = f64(o["G2"]).T @ f64(o["P"])
    if with_ba:
        got["dba"] = f64(o["bapart"]).sum().reshape(1, 1)
    else:
        assert not o["bapart"].any(), "bapart of a layer without an attention bias gradient"
    for k in names or got:
        ck(k, got[k], b64[k], e32[k], family)
    pad = torch.from_numpy(tab["eseg"] == 255).to(DEV)
    for k in ("G2", "P", "G1"):
        assert not o[k][pad].any(), f"{ck.what}: {k} is not zero on padding rows"
    for k in ("dx", "dx0"):
        assert not o[k][:, 3].any(), f"{ck.what}: fourth component of {k}"


def has_ba(variant, coord):
    return not coord and variant != "plainhead"


def handle_of(H, variant):
    return handle(H, variant if VARIANTS[variant][0] else "plain")


# ----------------------------------------------------------------------------- 1. forward, exact fp32
@pytest.mark.parametrize("coord", [0, 1])
@pytest.mark.parametrize("batch,H", CASES)
def test_forward_fp32(batch, H, coord):
    """Every node's row of `out` against the restatement; nodes without edges exactly 0 (a zero reference row must be zero);
    where the forward can keep pre2, keeping it does not change a bit of `out`."""
    r64, e32 = reference(batch, H, coord)
    dyn, tab = handle(H), table(batch)
    topo = topology(dyn, batch)
    d = device_inputs(inputs(batch, H, "plain"))
    out, _ = forward(dyn, topo, tab, coord, d)
    ck = Checker(batch, H, f"{batch} H={H} coord={coord} forward")
    ck("out", out, r64["out"], e32["out"])
    if batch == "wide":
        lonely = ~np.isin(np.arange(tab["M"]), tab["ei"][tab["eseg"] != 255])
        assert lonely.any() and not r64["out"][lonely].any() and not out[torch.from_numpy(lonely).to(DEV)].any()
    rows = save_rows(dyn, topo)
    if H >= 128:
        assert (rows == 0) == (batch in ("small", "wide"))
    else:
        assert rows == tab["rows"] + 32
    if rows:
        kept, pre2 = forward(dyn, topo, tab, coord, d, keep=True)
        assert torch.equal(kept, out) and not torch.isnan(pre2[:tab["rows"]]).any()
    ck.done()


# ----------------------------------------------------------------------------- 2. backward, exact fp32, recomputing
@pytest.mark.parametrize("coord", [0, 1])
@pytest.mark.parametrize("batch,H", CASES)
def test_backward_fp32_recomputing(batch, H, coord):
    """hd_edge_layer_backward for a random gout and for one that is zero outside one molecule: G2, P, G1, escal per edge row
    (exactly zero on padding rows and where the gradient is zero: a zero reference row must be zero), dAB, dx, dx0 per node, the
    per-tile partials and G2^T P summed on the host.  Two calls give identical bits."""
    r64, e32 = reference(batch, H, coord)
    dyn, tab = handle(H), table(batch)
    topo = topology(dyn, batch)
    d = device_inputs(inputs(batch, H, "plain"))
    ck = Checker(batch, H, f"{batch} H={H} coord={coord} backward")
    for k, gout in enumerate(gouts(batch, H, coord)):
        o = backward(dyn, topo, tab, coord, d, gout)
        ck.what = f"{batch} H={H} coord={coord} backward gout {k}"
        check_backward(ck, o, dict(r64["bwd"][k], P=r64["P"]), dict(e32["bwd"][k], P=e32["P"]), tab, coord, has_ba("plain", coord))
        if k == 0:
            assert_same_bits(o, backward(dyn, topo, tab, coord, d, gout), coord, ck.what + " second call")
    ck.done()


# ----------------------------------------------------------------------------- 3. kept pre2 equals recomputing
@pytest.mark.parametrize("coord", [0, 1])
@pytest.mark.parametrize("batch,H", KEPT)
def test_kept_pre2_equals_recomputing_bit_for_bit(batch, H, coord):
    """include/hierdiff_hip.h: "same results to the bit" - per row, per partial, per node, not only in the final gradients."""
    dyn, tab = handle(H), table(batch)
    topo = topology(dyn, batch)
    d = device_inputs(inputs(batch, H, "plain"))
    assert save_rows(dyn, topo) == tab["rows"] + 32
    _, pre2 = forward(dyn, topo, tab, coord, d, keep=True)
    for k, gout in enumerate(gouts(batch, H, coord)):
        a = backward(dyn, topo, tab, coord, d, gout)
        b = backward(dyn, topo, tab, coord, d, gout, pre2=pre2)
        assert_same_bits(a, b, coord, f"{batch} H={H} coord={coord} gout {k}: recomputing vs kept pre2")


# ----------------------------------------------------------------------------- 4. inputs the model cannot produce
@pytest.mark.parametrize("coord", [0, 1])
@pytest.mark.parametrize("variant", [v for v in VARIANTS if v != "plain"])
@pytest.mark.parametrize("batch,H", ODD)
def test_inputs_the_model_cannot_produce(batch, H, variant, coord):
    """x0 far from x; first-layer pre-activations deep in SiLU saturation (finite outputs); norm_constant = 1 (0 is every other
    test's handle: WIDE's self edge has radial = 0 there); attention without a bias pointer (= ba 0, bit for bit); attention and
    tanh off; aggregation_method 'mean'.  Forward and backward, the bars of every other test."""
    r64, e32 = reference(batch, H, coord, variant)
    dyn, tab = handle_of(H, variant), table(batch)
    topo = topology(dyn, batch)
    inp = inputs(batch, H, variant)
    d = device_inputs(inp)
    if variant == "noba":
        d["ba"] = None
    ck = Checker(batch, H, f"{batch} H={H} coord={coord} {variant} forward")
    out, _ = forward(dyn, topo, tab, coord, d)
    assert torch.isfinite(out).all()
    ck("out", out, r64["out"], e32["out"])
    if variant == "saturate":
        valid = tab["eseg"] != 255
        pre1 = inp["AB"][tab["ei"][valid], :H] + inp["AB"][tab["ej"][valid], H:]
        assert (np.abs(pre1).max(1) > 50).mean() > 0.05
    gout = gouts(batch, H, coord)[0]
    o = backward(dyn, topo, tab, coord, d, gout)
    ck.what = f"{batch} H={H} coord={coord} {variant} backward"
    check_backward(ck, o, dict(r64["bwd"][0], P=r64["P"]), dict(e32["bwd"][0], P=e32["P"]), tab, coord, has_ba(variant, coord))
    assert all(torch.isfinite(v).all() for v in defined(o, coord).values())
    if variant == "noba":
        d0 = dict(d, ba=torch.zeros(1, device=DEV))
        assert torch.equal(forward(dyn, topo, tab, coord, d0)[0], out)
        assert_same_bits(backward(dyn, topo, tab, coord, d0, gout), o, coord, "ba = 0 vs ba = NULL")
    ck.done()


# ----------------------------------------------------------------------------- 5. the fp16x3 training form
@pytest.mark.parametrize("coord", [0, 1])
@pytest.mark.parametrize("batch,H", [(b, H) for b in ("whole", "mixed") for H in (128, 256)])
def test_fp16x3_training_form(batch, H, coord):
    """hd_edge_layer_forward_s(precision 3, pre2) (k_edge with HD_EDGE_UNSCALED) and hd_edge_layer_backward_s(precision 3, pre2,
    f16ws) (stage B PREC 3) against float64, and the maxima the two stages leave in f16ws - per 128-row workgroup block max |G2| and
    max |P|, "exact, not a bound": as multisets, the workgroup-to-block map being the XCD bijection."""
    r64, e32 = reference(batch, H, coord)
    dyn, tab = handle(H), table(batch)
    topo = topology(dyn, batch)
    d = device_inputs(inputs(batch, H, "plain"))
    assert save_rows(dyn, topo, 3) == tab["rows"] + 32
    out, pre2 = forward(dyn, topo, tab, coord, d, prec=3, keep=True)
    ck = Checker(batch, H, f"{batch} H={H} coord={coord} fp16x3")
    ck("out", out, r64["out"], e32["out"], "X")
    o = backward(dyn, topo, tab, coord, d, gouts(batch, H, coord)[0], prec=3, pre2=pre2)
    check_backward(ck, o, dict(r64["bwd"][0], P=r64["P"]), dict(e32["bwd"][0], P=e32["P"]), tab, coord, has_ba("plain", coord), "X",
                   names=("G1", "dAB", "dx", "dx0"))
    n_wg = o["n_wg"]
    assert n_wg == tab["rows"] // 128
    for k, at in (("G2", 4), ("P", 4 + n_wg)):
        host = o[k].abs().reshape(n_wg, -1).max(1).values.sort().values
        assert torch.equal(host, o["f16ws"][at:at + n_wg].sort().values), f"per-workgroup maxima of |{k}|"
    ck.done()


@pytest.mark.parametrize("H", [128, 256])
def test_fp16x3_needs_the_kept_pre2(H):
    """Where the column-split kernels run the forward (SMALL), nothing is kept in precision 3 either, and a precision-3 backward
    without pre2 is refused on the host."""
    L, lib = _lib()
    dyn, tab = handle(H), table("small")
    topo = topology(dyn, "small")
    assert save_rows(dyn, topo, 3) == 0
    d = device_inputs(inputs("small", H, "plain"))
    assert backward(dyn, topo, tab, 0, d, gouts("small", H, 0)[0], prec=3, want_rc=True) < 0
    assert "precision 3" in lib.hd_last_error().decode()


# ----------------------------------------------------------------------------- 6. no edges
@pytest.mark.parametrize("coord", [0, 1])
def test_batch_without_edges(coord):
    """[1, 1, 1]: three active nodes, no edge.  The forward writes zeros, the backward zero-fills every output and workspace."""
    H = 64
    dyn = handle(H)
    nm, em = orc.canonical_masks([1, 1, 1])
    tab = elr.layout(nm.numpy()[..., 0], em.numpy())
    assert (tab["M"], tab["E"], tab["tiles"], tab["rows"]) == (3, 0, 1, 32)
    topo = dyn.topology(nm.to(DEV), em.to(DEV), 3, 1)
    assert topo.info()["tiles"] == 0
    d = device_inputs(elr.draw_inputs(3, H, 5))
    out, _ = forward(dyn, topo, tab, coord, d)
    assert not out.any()
    o = backward(dyn, topo, tab, coord, d, np.ones((3, 4 if coord else H)))
    for k in WS:
        assert not o[k].any(), k            # (any() is true for NaN: nothing is left unwritten)


# ----------------------------------------------------------------------------- 7. host-side refusals
def test_host_side_refusals():
    """No kernel runs: return code < 0 and hd_last_error."""
    L, lib = _lib()
    H = 32
    dyn, tab = handle(H), table("small")
    topo = topology(dyn, "small")
    d = device_inputs(inputs("small", H, "plain"))
    gout = gouts("small", H, 0)[0]
    last = lambda: lib.hd_last_error().decode()
    args = lambda dd: [_p(dd[k]) for k in ("AB", "x", "x0", "wrd", "W2", "b2", "wa", "ba")]
    out = _nan(tab["M"], H)
    fwd = lambda hd, tp, dd, prec=0: lib.hd_edge_layer_forward_s(hd._handle(), tp.ptr, 0, prec, *args(dd), _p(out), None, None)
    # null tensor
    assert fwd(dyn, topo, dict(d, AB=None)) < 0 and "null tensor" in last()
    assert backward(dyn, topo, tab, 0, dict(d, W2=None), gout, want_rc=True) < 0 and "null tensor" in last()
    # topology of another handle
    other = handle(H, "nc1")
    assert fwd(other, topo, d) < 0 and "another handle" in last()
    assert lib.hd_edge_layer_backward(other._handle(), topo.ptr, 0, *args(d), _p(out), *[_p(out)] * 11, None) < 0 and "another handle" in last()
    # a handle whose precision is not 0
    f16 = handle(H, "plain", "fp16x3")
    t16 = topology(f16, "small")
    assert fwd(f16, t16, d) < 0 and "precision 0" in last()
    assert backward(f16, t16, tab, 0, d, gout, want_rc=True) < 0 and "precision 0" in last()
    # precision 2 (retired), precision 3 without pre2 / f16ws
    assert fwd(dyn, topo, d, prec=2) < 0 and "precision must be 0" in last()
    assert backward(dyn, topo, tab, 0, d, gout, prec=2, want_rc=True) < 0 and "precision must be 0" in last()
    assert backward(dyn, topo, tab, 0, d, gout, prec=3, want_rc=True) < 0 and "needs the kept pre2" in last()
    pre2 = _nan(save_rows(dyn, topo), H)
    o = [_p(_nan(1))] * 11
    assert lib.hd_edge_layer_backward_s(dyn._handle(), topo.ptr, 0, 3, *args(d), _p(out), _p(pre2), None, *o, None) < 0
    assert "f16ws" in last()
    assert torch.isnan(out).all()           # nothing ran
    torch.cuda.synchronize()
