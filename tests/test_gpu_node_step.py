"""GPU tier: the node side of the forward on its own - hd_node_step through the C ABI against the float64 restatement of one node
step (tests/node_step_reference.py), tensor by tensor and row by row, on every path node_path() (csrc/launch.hpp) can take.

Bars (tests/node_step_reference.py, EXPERIMENTS.md section AX): per family of tensors the kernels' per-row error against float64
is at most `margin x the error of the float32 CPU evaluation of the same graph on the same case`, and beside it the suite's outer
bar, rel-L2 < 1e-4 per tensor (tests/helpers.py).

Batches (rows asserted by tests/test_node_step_cpu.py; the path asserted here from *path, so that a changed size rule does not
quietly test another kernel):
  SMALL      [5, 17, 30]       52 rows    two 32-row tiles, the second ragged; three 16-row groups + 4 rows; grid rounded up to 8
  WIDE       [70, 40, 3, 1]    N = 70, a general mask: a self edge, an asymmetric hole, a node with 138 incident edges (four part
                               rows, the most this batch has), a node with none, an active row with mask 0
  LONG       [200]             200 rows, 199 incident edges per node: seven or eight part rows behind every neighbour sum
  F16_BELOW  68 x [30] + [7]   2,047 rows fp16x3: k_node_split         F16_AT   68 x [30] + [8]    2,048 rows  fp16x3: k_node
  F32_BELOW  179 x [30] + [29] 5,399 rows fp32: the small-row chains   F32_AT   SMALL + 179 x [30] 5,422 rows  k_node_f32, ragged
Paths: 0 k_node_split, 1 k_node_split_f32, 2 k_node / k_node_f32, 3 the k_gemm_r16 chain.  Every output is NaN before a call.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import node_step_reference as nsr
from tests.helpers import assert_parity
from tests.test_gpu_parity import DEV, build_dynamics

pytestmark = pytest.mark.gpu

SPLIT, SPLIT_F32, FUSED, R16 = 0, 1, 2, 3
MODES = [("fp32", 32), ("fp32", 64), ("fp32", 128), ("fp32", 256), ("fp16x3", 128), ("fp16x3", 256), ("fp16x3", 64)]
BIG = [("fp32", 64, "f32_below"), ("fp32", 64, "f32_at"), ("fp32", 256, "f32_below"), ("fp32", 256, "f32_at"),
       ("fp16x3", 256, "f16_below"), ("fp16x3", 256, "f16_at"), ("fp16x3", 64, "f16_below"), ("fp16x3", 64, "f16_at"),
       ("fp32", 256, "f16_at"), ("fp16x3", 256, "f32_at")]
VARIANT_MODES = [("fp32", 64), ("fp32", 256), ("fp16x3", 128), ("fp16x3", 256)]
RATIOS = {}       # (family, precision, batch, H, variant) -> worst err(kernel) / err(float32 CPU) seen in this process (EXPERIMENTS.md section AX)


def expected_path(precision, H, M):
    """The issue's table, not the library's constants: fp16x3 node kernels exist at widths >= 128 and split below 2,048 rows; the
    fp32 node kernels fuse from 5,400 rows, below that widths >= 128 run k_node_split_f32 and narrower ones k_gemm_r16."""
    if precision == "fp16x3" and H >= 128:
        return SPLIT if M < 2048 else FUSED
    if M >= 5400:
        return FUSED
    return SPLIT_F32 if H >= 128 else R16


def is_f16(precision, H):
    return precision == "fp16x3" and H >= 128


# ----------------------------------------------------------------------------- handles, topologies, calls
def _kind(variant):
    return variant if variant in ("mean", "negbias") else "plain"


@functools.lru_cache(maxsize=None)
def handle(H, precision, kind="plain"):
    kw = dict(aggregation_method="mean") if kind == "mean" else {}
    dyn = build_dynamics(nsr.state_dict(H, kind), H, nsr.N_LAYERS, inv_sublayers=nsr.SUBLAYERS,
                         normalization_factor=nsr.NORMALIZATION_FACTOR, **kw)
    dyn.precision = precision
    dyn.sync_weights()
    return dyn


@functools.lru_cache(maxsize=None)
def _device_masks(batch):
    nm, em = nsr.masks(batch)
    return nm.contiguous().to(DEV), em.contiguous().to(DEV)


def topology(dyn, batch):
    nm, em = _device_masks(batch)
    topo = dyn.topology(nm, em, nm.shape[0], nm.shape[1])
    info, tab = topo.info(), nsr.table(batch)
    assert info["nodes"] == tab["M"] and info["parts"] == tab["parts"]
    return topo


def _lib():
    from hierdiff_amd import _lib as L
    return L, L.load()


def _dev(a):
    return torch.tensor(np.asarray(a), dtype=torch.float32, device=DEV).contiguous()


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV, dtype=torch.float32)


def _p(t):
    return None if t is None else t.data_ptr()


def step(dyn, topo, tab, layer, h, part, H, with_abmax, n_img, alias=False):
    """One hd_node_step call on device tensors; every output NaN before it.  Returns (device tensors, path)."""
    L, lib = _lib()
    M = tab["M"]
    out = dict(h=h.clone() if alias else _nan(M, H), AB=[_nan(M, 2 * H) for _ in range(n_img)],
               abmax=[_nan(M, 2) for _ in range(n_img)] if with_abmax else [])
    ab = [_p(t) for t in out["AB"]] + [None] * (2 - n_img)
    mx = [_p(t) for t in out["abmax"]] + [None] * (2 - len(out["abmax"]))
    path = C.c_int(-1)
    h_in = out["h"] if alias else h
    L.check(lib.hd_node_step(dyn._handle(), topo.ptr, layer, _p(h_in), _p(part), _p(out["h"]), ab[0], ab[1], mx[0], mx[1],
                             C.byref(path), None), "hd_node_step")
    torch.cuda.synchronize()
    return out, path.value


def host(out):
    f = lambda t: t.double().cpu().numpy()
    return dict(h=f(out["h"]), AB=[f(t) for t in out["AB"]], abmax=[f(t) for t in out["abmax"]])


def same_bits(a, b, what, rows=None):
    for k in ("h", "AB", "abmax"):
        for q, (x, y) in enumerate(zip(a[k] if k != "h" else [a[k]], b[k] if k != "h" else [b[k]])):
            x, y = (x, y) if rows is None else (x[:rows], y[:rows])
            assert torch.equal(x, y), f"{what}: {k}{q} differs, max {(x - y).abs().max().item():.3e}"


def run_case(precision, H, batch, variant, layers):
    """Every contract of nsr.check on the layers given, and the path."""
    dyn, tab = handle(H, precision, _kind(variant)), nsr.table(batch)
    topo = topology(dyn, batch)
    f16, with_abmax = is_f16(precision, H), precision == "fp16x3"
    scaled = precision == "fp16x3"          # the edge model's scaled domain: part rows and AB carry c = -log2(e)
    inp = nsr.inputs(batch, H, variant, scaled)
    h, part = _dev(inp["h"]), _dev(inp["part"])
    failed = []
    for layer in layers:
        r64, e32 = nsr.reference(batch, H, variant, layer, scaled)
        w = nsr.layer_weights(nsr.state_dict(H, _kind(variant)), layer, scaled)
        out, path = step(dyn, topo, tab, layer, h, part, H, with_abmax, len(w["nxt"]))
        assert path == expected_path(precision, H, tab["M"]), f"path {path}"
        got = host(out)
        what = f"{batch} H={H} {precision} {variant} layer {layer}"
        key = (precision, batch, H, variant)
        bad = nsr.check(got, r64, e32, tab, w, f16, with_abmax, RATIOS, key)
        for name, g, r, e in [("h", got["h"], r64["h"], e32["h"])] + [(f"AB{q}", got["AB"][q], r64["AB"][q], e32["AB"][q])
                                                                      for q in range(len(r64["AB"]))]:
            eg = nsr.err(g, r)
            print(f"{what} {name}: err {eg:.3e}  float32 CPU {e:.3e}  ratio {eg / max(e, nsr.YARDSTICK_FLOOR):.2f}  "
                  f"(margin {nsr.MARGINS[nsr.family(name, f16)]:g})")
            try:
                assert_parity(g, r, f"{what} {name}")
            except AssertionError as ex:
                bad.append(str(ex))
        failed += [f"layer {layer}: {b}" for b in bad]
    assert not failed, f"{batch} H={H} {precision} {variant}:\n  " + "\n  ".join(failed)


# ----------------------------------------------------------------------------- 1. accuracy, masked rows, row maxima: every path
@pytest.mark.parametrize("batch", ["small", "wide"])
@pytest.mark.parametrize("precision,H", MODES)
def test_small_batches_every_width(precision, H, batch):
    """Layers -1, 0 and 1 on the ragged 52-row batch and on the general mask: h' and every AB per row, a masked active row exactly
    {0, [b1 | 0]}, abmax the row maxima of the AB of the same call, bit for bit."""
    run_case(precision, H, batch, "plain", nsr.LAYERS)


@pytest.mark.parametrize("precision,H,batch", BIG)
def test_size_thresholds(precision, H, batch):
    """One row under and at the two size thresholds: the three-launch chains and the fused kernels, full and ragged last tiles."""
    run_case(precision, H, batch, "plain", nsr.LAYERS)


@pytest.mark.parametrize("variant", ["plain", "mean"])
@pytest.mark.parametrize("precision,H", VARIANT_MODES)
def test_long_part_chains(precision, H, variant):
    """Seven or eight partial sums per node (WIDE has at most four): a dropped or doubled last part shows per row."""
    assert np.diff(nsr.table("long")["pstart"]).min() >= 7
    run_case(precision, H, "long", variant, (0, 1))


def test_all_four_paths_are_reached():
    M = {b: nsr.table(b)["M"] for b in nsr.BATCHES}
    seen = {expected_path(p, H, M[b]) for p, H, b in BIG} | {expected_path(p, H, M["small"]) for p, H in MODES}
    assert seen == {SPLIT, SPLIT_F32, FUSED, R16}
    assert expected_path("fp16x3", 256, M["f16_below"]) == SPLIT and expected_path("fp16x3", 256, M["f16_at"]) == FUSED
    assert expected_path("fp32", 256, M["f32_below"]) == SPLIT_F32 and expected_path("fp32", 64, M["f32_below"]) == R16
    assert expected_path("fp32", 64, M["f32_at"]) == FUSED == expected_path("fp32", 256, M["f32_at"])


# ----------------------------------------------------------------------------- 2. inputs where ranged operands or the sum go wrong
@pytest.mark.parametrize("variant", [v for v in nsr.VARIANTS if v != "plain"])
@pytest.mark.parametrize("batch", ["small", "wide"])
@pytest.mark.parametrize("precision,H", VARIANT_MODES)
def test_inputs_that_strain_the_row_ranges(precision, H, batch, variant):
    """mean aggregation; a row bound 2^12 above typical elements; max |h| << max |X|; X = 0 (row bound 0: T = SiLU(b3), finite);
    rows at 2^-60; T ~ 0 under a large bound.  The two-image step (layer 1) and the AB-only step, the bars of every other test."""
    run_case(precision, H, batch, variant, (-1, 1))


# ----------------------------------------------------------------------------- 3. row locality
@pytest.mark.parametrize("precision,H", MODES)
def test_head_rows_do_not_depend_on_the_batch_or_the_path(precision, H):
    """SMALL's molecules head F32_AT with the same rows of h and part: their 52 rows of h', AB and abmax are the same bits on the
    small-batch path and on the fused kernel."""
    dyn = handle(H, precision)
    with_abmax = precision == "fp16x3"
    res = {}
    for batch in ("small", "f32_at"):
        tab, inp = nsr.table(batch), nsr.inputs(batch, H, "plain", with_abmax)
        topo = topology(dyn, batch)
        res[batch] = [step(dyn, topo, tab, layer, _dev(inp["h"]), _dev(inp["part"]), H, with_abmax, 2 if layer == 1 else 1)
                      for layer in nsr.LAYERS]
    small, big = (nsr.inputs(b, H, "plain", with_abmax) for b in ("small", "f32_at"))
    assert np.array_equal(big["h"][:52], small["h"]) and np.array_equal(big["part"][:len(small["part"])], small["part"])
    for k, layer in enumerate(nsr.LAYERS):
        (a, pa), (b, pb) = res["small"][k], res["f32_at"][k]
        assert pa == expected_path(precision, H, 52) != FUSED and pb == FUSED
        same_bits(a, b, f"H={H} {precision} layer {layer}: small batch vs fused", rows=52)


# ----------------------------------------------------------------------------- 4. repeatability, aliasing
@pytest.mark.parametrize("batch", ["small", "f16_at"])
@pytest.mark.parametrize("precision,H", [("fp32", 64), ("fp32", 256), ("fp16x3", 256)])
def test_two_calls_and_aliased_rows_give_the_same_bits(precision, H, batch):
    with_abmax = precision == "fp16x3"
    dyn, tab, inp = handle(H, precision), nsr.table(batch), nsr.inputs(batch, H, "plain", with_abmax)
    topo = topology(dyn, batch)
    h, part = _dev(inp["h"]), _dev(inp["part"])
    for layer in nsr.LAYERS:
        n_img = 2 if layer == 1 else 1
        a, _ = step(dyn, topo, tab, layer, h, part, H, with_abmax, n_img)
        b, _ = step(dyn, topo, tab, layer, h, part, H, with_abmax, n_img)
        c, _ = step(dyn, topo, tab, layer, h, part, H, with_abmax, n_img, alias=True)
        assert not any(torch.isnan(t).any() for t in [a["h"]] + a["AB"] + a["abmax"])
        same_bits(a, b, f"{batch} H={H} {precision} layer {layer}: second call")
        same_bits(a, c, f"{batch} H={H} {precision} layer {layer}: h_out == h_in")
        assert torch.equal(h, _dev(inp["h"]))           # the non-aliased calls left h_in alone


# ----------------------------------------------------------------------------- 5. documented refusals
def test_documented_refusals():
    """Return code < 0, hd_node_step in hd_last_error, nothing written, and the next valid call works."""
    L, lib = _lib()
    H = 64
    dyn, tab, inp = handle(H, "fp32"), nsr.table("small"), nsr.inputs("small", H)
    topo = topology(dyn, "small")
    h, part = _dev(inp["h"]), _dev(inp["part"])
    M = tab["M"]
    ho, ab0, ab1, mx = _nan(M, H), _nan(M, 2 * H), _nan(M, 2 * H), _nan(M, 2)
    path = C.c_int(-1)
    last = lambda: lib.hd_last_error().decode()

    def call(hd=dyn, tp=topo, layer=1, h_in=h, prt=part, h_out=ho, a0=ab0, a1=ab1, m0=None, m1=None, pth=path):
        return lib.hd_node_step(None if hd is None else hd._handle(), None if tp is None else tp.ptr, layer, _p(h_in), _p(prt), _p(h_out),
                                _p(a0), _p(a1), _p(m0), _p(m1), None if pth is None else C.byref(pth), None)

    def refused(rc, words):
        assert rc < 0 and "hd_node_step" in last() and words in last(), (rc, last())
        torch.cuda.synchronize()
        assert all(torch.isnan(t).all() for t in (ho, ab0, ab1, mx)) and path.value == -1      # nothing written
        assert call() == 0                              # the handle is still usable
        torch.cuda.synchronize()
        assert not any(torch.isnan(t).any() for t in (ho, ab0, ab1)) and path.value == R16
        for t in (ho, ab0, ab1):
            t.fill_(float("nan"))
        path.value = -1

    refused(call(hd=None), "null handle")
    refused(call(tp=None), "null handle/topology")
    for k in ("h_in", "h_out", "a0", "prt", "pth"):
        refused(call(**{k: None}), "null tensor")
    for layer in (-2, nsr.N_LAYERS * nsr.SUBLAYERS, 1 << 20):
        refused(call(layer=layer), "layer out of range")
    other = handle(H, "fp32", "mean")
    refused(call(hd=other), "another handle")
    refused(call(a1=None), "ab1 missing")
    refused(call(m0=mx), "precision 0")
    refused(call(layer=0, m1=mx), "precision 0")
    # weights not set: a fresh handle of the same configuration that nothing has packed its parameters into
    bare = build_dynamics(nsr.state_dict(H), H, nsr.N_LAYERS, inv_sublayers=nsr.SUBLAYERS)
    refused(call(hd=bare, tp=topology(bare, "small")), "weights not set")
    # what is allowed: part NULL with layer -1, ab1 ignored where one image is written
    assert call(layer=-1, prt=None, a1=None) == 0
    torch.cuda.synchronize()
    assert torch.equal(ho, h) and not torch.isnan(ab0).any() and path.value == R16
