"""CPU tier: the float64 restatement of one edge layer (tests/edge_layer_reference.py) is the reference's layer, its
parameter-level sums are autograd's, and the margins committed for the GPU tier (tests/test_gpu_edge_layer.py) reject every
mutant of the restatement."""
import functools

import numpy as np
import pytest
import torch

from oracle import egnn_oracle as orc
from tests import edge_layer_reference as elr

H = 32


def general_masks():
    """The masks of test_general_edge_mask_and_options_vs_oracle: disconnected blocks, a self edge, an asymmetric hole."""
    nm, em = orc.canonical_masks([9, 6, 12], 12)
    em = em.clone()
    em[0, :4, 4:9] = False; em[0, 4:9, :4] = False
    em[1, 2, 2] = True
    em[2, 0, 1] = False
    return nm.numpy()[..., 0], em.numpy()


def canonical():
    nm, em = orc.canonical_masks([5, 17, 30])
    return nm.numpy()[..., 0], None, em.numpy()


@functools.lru_cache(maxsize=None)
def _case(which):
    if which == "general":
        nm, em = general_masks()
        tab = elr.layout(nm, em)
    else:
        nm, _, em = canonical()
        tab = elr.layout(nm, None)
    inp = elr.draw_inputs(tab["M"], H, 11)
    return nm, em, tab, inp


def oracle_layer(inp, nm, em, tab, opts, coord, aggregation_method):
    """agg of oracle._gcl / (x' - x) of oracle._equivariant_update in float64 on the dense [B N^2] edge list, compact node rows."""
    B, N = nm.shape
    t64 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))
    idx = torch.from_numpy(tab["node_of"])
    flat = lambda a: torch.zeros((B * N, a.shape[1]), dtype=torch.float64).index_copy(0, idx, t64(a))
    h, x, x0 = flat(inp["h"]), flat(inp["x"][:, :3]), flat(inp["x0"][:, :3])
    row, col = orc.edge_index(N, B)
    node_mask, edge_mask = t64(nm).reshape(B * N, 1), t64(em).reshape(B * N * N, 1)
    cfg = orc.DynCfg(hidden_nf=H, n_layers=1, attention=opts.attention, tanh=opts.tanh, norm_constant=opts.norm_constant,
                     normalization_factor=opts.norm, coords_range=opts.coords_range, aggregation_method=aggregation_method)
    radial, coord_diff = orc._coord2diff(x, row, col, cfg.norm_constant)
    d0, _ = orc._coord2diff(x0, row, col, 1.0)
    edge_attr = torch.cat([radial, d0], dim=1)
    first = "coord_mlp" if coord else "edge_mlp"
    sd = {f"{first}.0.weight": t64(inp["W1"]), f"{first}.0.bias": t64(inp["b1"]), f"{first}.2.weight": t64(inp["W2"]),
          f"{first}.2.bias": t64(inp["b2"])}
    with torch.no_grad():
        if coord:
            sd["coord_mlp.4.weight"] = t64(inp["wa"])[None]
            xn = orc._equivariant_update(sd, "", h, x, row, col, coord_diff, edge_attr, torch.ones_like(node_mask), edge_mask, cfg)
            return (xn - x)[idx].numpy()
        sd.update({"att_mlp.0.weight": t64(inp["wa"])[None], "att_mlp.0.bias": t64(inp["ba"]),
                   "node_mlp.0.weight": torch.zeros(H, 2 * H, dtype=torch.float64), "node_mlp.0.bias": torch.zeros(H, dtype=torch.float64),
                   "node_mlp.2.weight": torch.zeros(H, H, dtype=torch.float64), "node_mlp.2.bias": torch.zeros(H, dtype=torch.float64)})
        return orc._gcl(sd, "", h, row, col, edge_attr, node_mask, edge_mask, cfg)[1][idx].numpy()


@pytest.mark.parametrize("coord", [False, True])
@pytest.mark.parametrize("which,attention,tanh,nc,method", [
    ("canonical", True, True, 0.0, "sum"),
    ("general", True, True, 1.0, "sum"),
    ("general", True, True, 0.0, "sum"),
    ("canonical", True, True, 0.0, "mean"),
    ("general", False, False, 1.0, "sum"),
])
def test_the_restatement_is_the_reference_layer(which, attention, tanh, nc, method, coord):
    nm, em, tab, inp = _case(which)
    inp = dict(inp, AB=elr.first_linear(inp["h"], inp["W1"], inp["b1"]))
    opts = elr.Opts(attention=attention, tanh=tanh, norm_constant=nc, coords_range=30.0,
                    norm=float(nm.shape[1]) if method == "mean" else 10.0)
    got = elr.edge_layer(inp, tab, opts, coord)["out"]
    ref = oracle_layer(inp, nm, em, tab, opts, coord, method)
    assert np.abs(ref).max() > 1e-3
    assert np.abs(got[:, :ref.shape[1]] - ref).max() <= 1e-12 * np.abs(ref).max()
    assert not got[:, ref.shape[1]:].any()                 # fourth component of a coordinate layer


@pytest.mark.parametrize("coord", [False, True])
@pytest.mark.parametrize("which", ["canonical", "general"])
def test_parameter_level_sums_equal_autograd(which, coord):
    """dW2 = G2^T P, db2 = colsum(G2), d(w_r), d(w_d) = {radial, d0}^T G1 - the sums a caller of hd_edge_layer_backward forms -
    and d(wa), d(ba), which leave the kernels as per-tile partial sums of quantities the restatement gets from autograd."""
    nm, em, tab, inp = _case(which)
    gout = np.random.default_rng(3).standard_normal((tab["M"], 4 if coord else H))
    r = elr.edge_layer(inp, tab, elr.Opts(norm_constant=1.0), coord, gouts=[gout])
    b = r["bwd"][0]
    for name in ("dW2", "db2", "dwrd"):
        assert np.abs(b[name]).max() > 0
        assert np.abs(b[name + "_rows"] - b[name]).max() <= 1e-12 * np.abs(b[name]).max(), name
    assert np.abs(b["G2"].T @ r["P"] - b["dW2"]).max() <= 1e-12 * np.abs(b["dW2"]).max()
    assert np.abs(b["dwa"]).max() > 0 and (coord or abs(b["dba"]).max() > 0)
    # padding rows are zero in every per-row tensor
    pad = tab["eseg"] == 255
    assert pad.any() and not any(np.any(t[pad]) for t in (r["P"], b["G2"], b["G1"], b["escal_rd"]))


MUTANT_CASES = {        # mutant -> (masks, coordinate layer, norm_constant)
    "a": ("canonical", False, 0.0), "b": ("canonical", False, 0.0), "c": ("canonical", False, 0.0),
    "d": ("general", True, 0.0),    # the self edge: 0 / (sqrt(0 + 1e-8) + 0) = 0, without the 1e-8 0 / 0
    "e": ("general", True, 1.0), "f": ("canonical", True, 0.0), "g": ("canonical", False, 0.0), "h": ("canonical", False, 0.0),
}


def _flat(res):
    return dict(out=res["out"], P=res["P"], **{k: v for k, v in res["bwd"][0].items() if not k.endswith("_rows")})


@pytest.mark.parametrize("mutant", sorted(elr.MUTANTS))
def test_every_mutant_is_rejected_at_the_committed_margins(mutant):
    """err(mutant64, ref64) > margin x err(ref32, ref64) on at least one tensor the GPU tier checks, while the float32 evaluation
    itself passes every bar."""
    which, coord, nc = MUTANT_CASES[mutant]
    nm, em, tab, inp = _case(which)
    opts = elr.Opts(norm_constant=nc)
    gout = np.random.default_rng(5).standard_normal((tab["M"], 4 if coord else H))
    ref64 = _flat(elr.edge_layer(inp, tab, opts, coord, gouts=[gout]))
    ref32 = _flat(elr.edge_layer(inp, tab, opts, coord, gouts=[gout], float32=True))
    mut = _flat(elr.edge_layer(inp, tab, opts, coord, gouts=[gout], mutant=mutant))
    assert set(ref64) <= set(elr.FAMILY)
    caught = []
    for name, ref in ref64.items():
        e32 = elr.err(ref32[name], ref)
        assert e32 <= elr.bar(elr.FAMILY[name], e32), name
        if elr.err(mut[name], ref) > elr.bar(elr.FAMILY[name], e32):
            caught.append(name)
    assert caught, f"mutant ({mutant}) {elr.MUTANTS[mutant]}: passes every bar"
    if mutant == "h":
        assert caught == ["dAB"]


def test_error_measure():
    ref = np.array([[1.0, -4.0], [0.0, 0.0], [2.0, 0.0]])
    assert elr.err(ref, ref) == 0.0
    assert elr.err(ref + np.array([[0.0, 0.0], [0.0, 0.0], [0.0, 0.5]]), ref) == 0.25
    assert elr.err(ref + np.array([[0.0, 0.0], [0.0, 1e-30], [0.0, 0.0]]), ref) == float("inf")     # a zero row must stay zero
    assert elr.err(np.where(ref == 2.0, np.nan, ref), ref) == float("inf")
    assert elr.err(-0.0 * ref, 0.0 * ref) == 0.0
