"""Float64 restatement of ONE node step of the forward (include/hierdiff_hip.h, the comment above hd_node_step; the contract of
csrc/k_node.hpp, "fused node update").  TEST INFRASTRUCTURE ONLY.

Per active node row i of the topology's compact node order, with the node model of one GCL and the first edge Linear of the
layer(s) that follow it:

    agg_i = (sum of the node's part rows, pstart[i] .. pstart[i+1]-1, ascending) / norm      norm = normalization_factor, or N ('mean')
    X = [h | agg]
    T = SiLU(X W3^T + b3)                                   W3 = node_mlp.0.weight [H, 2H]
    h' = (h + T W4^T + b4) * mask                           W4 = node_mlp.2.weight [H, H]
    AB_q = h' [W1a_q | W1b_q]^T + [b1_q | 0]                W1 = edge_mlp.0.weight / coord_mlp.0.weight [H, 2H + 2], columns [a | b | r, d]
    abmax_q[r] = {max_k |A_r[k]|, max_k |B_r[k]|}

(layer -1: the last two lines only, on h as it is.)  Weights are taken from the state dict in its own layout.

A handle of precision 3 (fp16x3) runs its edge model in the domain scaled by c = -log2(e) (hd_set_weights): the part rows its edge
kernels leave are c x the neighbour sums and the AB they read is c x the above, with c folded into the packed weights, one float32
rounding per weight.  `scaled=True` states that: W3's agg half is divided by c, W1 and b1 are multiplied by c - exactly in float64,
rounded per weight in the float32 evaluation, as the library rounds them - and `inputs(.., scaled=True)` draws part rows c times as large.

`node_step`
evaluates this graph in float64 or, `float32=True`, the identical graph in float32 on the CPU: the yardstick the kernels' errors
are measured by.  The error measure, `bar` and YARDSTICK_FLOOR are those of tests/edge_layer_reference.py.

Domain: no case here uses values whose a-priori row bound (csrc/k_node.hpp: max|X_r| L1(W3) + max|b3| for T, max|h_r| + that times
L1(W4) + max|b4| for h') overflows fp32 - that is outside the kernels' stated domain.

Also here: the committed margins of tests/test_gpu_node_step.py, the batches, variants and seeded inputs both tiers use, and the
named one-line MUTANTS of the restatement that tests/test_node_step_cpu.py proves those margins reject.
"""
import ctypes as C
import functools
from typing import Dict, List, Optional

import numpy as np
import torch
import torch.nn.functional as F

from oracle import egnn_oracle as orc
from tests import edge_layer_reference as elr
from tests.edge_layer_reference import YARDSTICK_FLOOR, err  # noqa: F401  (one definition, used by both harnesses)

# ----------------------------------------------------------------------------- bars (EXPERIMENTS.md section AX)
# Families: NH h' and NA AB in exact fp32 | NX both tensors in fp16x3 (at widths below 128 the fp16x3 handle runs the fp32 node
# kernels and is held to NH / NA).  Each margin is twice the worst kernel-to-yardstick ratio measured on an MI355X, rounded up to
# a power of two (table in EXPERIMENTS.md section AX); a family that needed more than 32 would be a finding, not a wider bar.
MARGINS = {"NH": 4.0, "NA": 4.0, "NX": 2.0}


def bar(family: str, err32: float) -> float:
    return elr.bar(family, err32, MARGINS)


def family(name: str, f16: bool) -> str:
    return "NX" if f16 else ("NH" if name == "h" else "NA")


# ----------------------------------------------------------------------------- batches, model, variants
HEAD = [5, 17, 30]
BATCHES = {     # name -> (molecule sizes, padded N)
    "small": (HEAD, 30),
    "wide": ([70, 40, 3, 1], 70),
    "long": ([200], 200),           # 199 incident edges per node: seven or eight part rows behind every sum
    "f16_below": ([30] * 68 + [7], 30),
    "f16_at": ([30] * 68 + [8], 30),
    "f32_below": ([30] * 179 + [29], 30),
    "f32_at": (HEAD + [30] * 179, 30),
}
ROWS = {"small": 52, "long": 200, "f16_below": 2047, "f16_at": 2048, "f32_below": 5399, "f32_at": 5422}
N_LAYERS, SUBLAYERS = 2, 2
LAYERS = (-1, 0, 1)             # AB only | a mid-block GCL (one image) | block 0's last GCL with block 1 behind it (two images)
VARIANTS = ("plain", "mean", "spike", "quiet", "zero", "tiny", "negbias")
NORMALIZATION_FACTOR = 10.0
C_SCALED = -1.4426950408889634074       # -log2(e): the scaled domain of a precision-3 handle's edge model


@functools.lru_cache(maxsize=None)
def masks(batch):
    n_list, N = BATCHES[batch]
    nm, em = orc.canonical_masks(n_list, N)
    if batch == "wide":
        em = em.clone()
        em[1, 5, 5] = True          # a self edge
        em[0, 0, 1] = False         # an asymmetric hole
        em[2, 5, 0] = True          # an unmasked edge to a padded node: row (2, 5) is active, has a part row and carries mask 0
    return nm, em


@functools.lru_cache(maxsize=None)
def table(batch) -> Dict:
    """elr.layout plus what the node side reads: pstart [M + 1], parts, the node mask per compact row."""
    from hierdiff_amd import _lib
    nm, em = masks(batch)
    nm_np, em_np = nm.numpy()[..., 0], em.numpy()
    tab = dict(elr.layout(nm_np, em_np))
    lib = _lib.load()
    B, N = nm_np.shape
    nmb = np.ascontiguousarray(nm_np.reshape(B, N), dtype=np.uint8)
    emb = np.ascontiguousarray(em_np.reshape(B, N, N), dtype=np.uint8)
    counts = (C.c_longlong * 5)()
    pstart = np.zeros(tab["M"] + 1, np.int32)
    _lib.check(lib.hd_topology_layout(nmb.ctypes.data, emb.ctypes.data, B, N, counts, None, None, None, None, None,
                                      pstart.ctypes.data), "hd_topology_layout")
    tab["pstart"], tab["parts"] = pstart.astype(np.int64), int(counts[3])
    assert tab["parts"] == pstart[-1]
    tab["mask"] = nmb.reshape(-1)[tab["node_of"]].astype(np.float64)
    return tab


def zero_row(tab) -> int:
    """The compact row the `zero` variant makes X = 0 on: the node without edges (WIDE's one-atom molecule); in a batch that has
    none, row 0, whose part rows are zeroed with it."""
    rows = np.flatnonzero((np.diff(tab["pstart"]) == 0) & (tab["mask"] == 1))
    assert len(rows) <= 1
    return int(rows[0]) if len(rows) else 0


def state_dict(H: int, variant: str = "plain"):
    """synthetic_state_dict of the two-block model every case runs on; `negbias`: b3 of every GCL shifted by -40."""
    from hierdiff_amd.weights import synthetic_state_dict
    sd = synthetic_state_dict(9, 0, H, N_LAYERS, SUBLAYERS, True, 700 + H, 1.0)
    if variant == "negbias":
        for k in sd:
            if k.endswith("node_mlp.0.bias"):
                sd[k] = (sd[k] - 40.0).astype(np.float32)
    return sd


def layer_weights(sd, layer: int, scaled: bool = False) -> Dict:
    """W3, b3, W4, b4 of GCL `layer` (None for -1) and the first edge Linear (W1 [H, 2H + 2], b1) of the layers that follow it, by
    the forward's rule: the next sub-layer, or the block's coordinate layer and the next block's first GCL.  scaled: c folded in."""
    c = C_SCALED if scaled else 1.0
    g = lambda k: np.asarray(sd["dynamics.egnn." + k], dtype=np.float64)
    first = lambda p, mlp: (g(f"{p}.{mlp}.0.weight") * c, g(f"{p}.{mlp}.0.bias") * c)
    if layer < 0:
        return dict(node=None, nxt=[first("e_block_0.gcl_0", "edge_mlp")])
    i, j = divmod(layer, SUBLAYERS)
    p = f"e_block_{i}.gcl_{j}"
    node = dict(W3=g(p + ".node_mlp.0.weight"), b3=g(p + ".node_mlp.0.bias"), W4=g(p + ".node_mlp.2.weight"), b4=g(p + ".node_mlp.2.bias"))
    node["W3"][:, node["W3"].shape[0]:] /= c
    if j + 1 < SUBLAYERS:
        nxt = [first(f"e_block_{i}.gcl_{j + 1}", "edge_mlp")]
    else:
        nxt = [first(f"e_block_{i}.gcl_equiv", "coord_mlp")]
        if i + 1 < N_LAYERS:
            nxt.append(first(f"e_block_{i + 1}.gcl_0", "edge_mlp"))
    return dict(node=node, nxt=nxt)


def _f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def spike_rows(M: int) -> np.ndarray:
    return np.arange(0, M, 7)


@functools.lru_cache(maxsize=None)
def inputs(batch, H, variant="plain", scaled=False) -> Dict[str, np.ndarray]:
    """h [M, H] ~ N(0, 1) and part [parts, H] ~ 2 N(0, 1), times c with `scaled` (float64 arrays that hold float32 values).  The
    batches that start with the SMALL molecules carry SMALL's rows of both at their head (row locality)."""
    tab = table(batch)
    M, P = tab["M"], tab["parts"]
    rng = np.random.Generator(np.random.PCG64(4000 + H + len(BATCHES[batch][0])))
    h, part = rng.standard_normal((M, H)), 2.0 * rng.standard_normal((P, H))
    if batch != "small" and BATCHES[batch][0][:3] == HEAD:
        small, stab = inputs("small", H, "plain", False), table("small")
        assert np.array_equal(tab["pstart"][:stab["M"] + 1], stab["pstart"])
        h[:stab["M"]], part[:stab["parts"]] = small["h"], small["part"]
    ps = tab["pstart"]
    of = np.repeat(np.arange(M), np.diff(ps))           # the node of every part row
    tenth = np.arange(M) % 10 == 3
    if variant == "spike":                              # one element 2^12 times the rest: the row bound far above typical elements
        r = spike_rows(M)
        h[r, (5 * r) % H] *= 4096.0
    if variant == "quiet":                              # max |h| << max |X|
        h[tenth] *= 2.0 ** -10
        part[tenth[of]] *= 2.0 ** 7
    if variant == "tiny":
        h[tenth] *= 2.0 ** -60
        part[tenth[of]] *= 2.0 ** -60
    if variant == "zero":                               # X = 0: the row bound is 0
        h[zero_row(tab)] = 0.0
        part[of == zero_row(tab)] = 0.0
    return dict(h=_f32(h), part=_f32(_f32(part) * (C_SCALED if scaled else 1.0)))


def norm_of(batch, variant) -> float:
    return float(BATCHES[batch][1]) if variant == "mean" else NORMALIZATION_FACTOR


# ----------------------------------------------------------------------------- mutants
MUTANTS = {
    "lastpart": "the last part of a node with two or more parts is dropped",
    "nonorm": "/ norm omitted",
    "maskfirst": "the mask applied before the residual add instead of after",
    "b1both": "b1 added to the B half too",
    "swapab": "W1a and W1b swapped",
    "round11": "h' rounded to 11 significant bits before the AB product (a lost fp16 tail piece)",
    "spikeround": "X rounded to 11 significant bits on the spike rows only",
    "ragged": "rows from 32 * (M // 32) on left unwritten",
    "maxpremask": "ABmax taken before the mask",
}


def _round11(t):
    m, e = torch.frexp(t)
    return torch.ldexp(torch.round(m * 2048.0) / 2048.0, e)


# ----------------------------------------------------------------------------- the step
def node_step(inp: Dict[str, np.ndarray], tab: Dict, w: Dict, norm: float, float32: bool = False,
              mutant: Optional[str] = None) -> Dict:
    """h [M, H], AB: one [M, 2H] per following layer, abmax: one [M, 2] per AB, T [M, H] (None for an AB-only step); numpy float64
    arrays (of float32 values with float32=True)."""
    assert mutant is None or mutant in MUTANTS
    dt = torch.float32 if float32 else torch.float64
    tt = lambda a: torch.tensor(np.asarray(a), dtype=dt)
    h, mask = tt(inp["h"]), tt(tab["mask"])[:, None]
    M, H = h.shape
    T = None
    pre_mask = h
    if w["node"] is not None:
        ps = tab["pstart"]
        of = np.repeat(np.arange(M), np.diff(ps))
        keep = np.ones(len(of), dtype=bool)
        if mutant == "lastpart":
            keep[ps[1:][np.diff(ps) >= 2] - 1] = False
        part = tt(inp["part"])
        agg = torch.zeros((M, H), dtype=dt).index_add(0, torch.from_numpy(of[keep]), part[torch.from_numpy(keep)])
        if mutant != "nonorm":
            agg = agg / norm
        X = torch.cat([h, agg], dim=1)
        if mutant == "spikeround":
            r = torch.from_numpy(spike_rows(M))
            X[r] = _round11(X[r])
        n = {k: tt(v) for k, v in w["node"].items()}
        T = F.silu(X @ n["W3"].T + n["b3"])
        upd = T @ n["W4"].T + n["b4"]
        pre_mask = h + upd
        h = h * mask + upd if mutant == "maskfirst" else pre_mask * mask
    res = {"AB": [], "abmax": []}
    for W1, b1 in w["nxt"]:
        W1, b1 = tt(W1), tt(b1)
        Wa, Wb = (W1[:, H:2 * H], W1[:, :H]) if mutant == "swapab" else (W1[:, :H], W1[:, H:2 * H])
        first = lambda hh: torch.cat([hh @ Wa.T + b1, hh @ Wb.T + (b1 if mutant == "b1both" else 0.0)], dim=1)
        AB = first(_round11(h) if mutant == "round11" else h)
        src = first(pre_mask) if mutant == "maxpremask" else AB
        res["AB"].append(AB)
        res["abmax"].append(torch.stack([src[:, :H].abs().max(1).values, src[:, H:].abs().max(1).values], dim=1))
    res["h"], res["T"] = h, T
    f64 = lambda t: None if t is None else t.to(torch.float64).numpy().copy()
    res = {"h": f64(res["h"]), "T": f64(res["T"]), "AB": [f64(t) for t in res["AB"]], "abmax": [f64(t) for t in res["abmax"]]}
    if mutant == "ragged":
        for t in [res["h"]] + res["AB"] + res["abmax"]:
            t[32 * (M // 32):] = np.nan
    return res


@functools.lru_cache(maxsize=None)
def reference(batch, H, variant, layer, scaled=False):
    """(float64 results, per tensor the float32 CPU evaluation's error against them: {"h": e, "AB": [e, ..]})."""
    tab, inp = table(batch), inputs(batch, H, variant, scaled)
    w = layer_weights(state_dict(H, variant), layer, scaled)
    r64 = node_step(inp, tab, w, norm_of(batch, variant))
    r32 = node_step(inp, tab, w, norm_of(batch, variant), float32=True)
    for k in ("h", "AB", "abmax"):
        for a in (r64[k] if isinstance(r64[k], list) else [r64[k]]):
            a.setflags(write=False)
    return r64, errors(r32, r64)


def errors(got: Dict, r64: Dict) -> Dict:
    return {"h": err(got["h"], r64["h"]), "AB": [err(g, r) for g, r in zip(got["AB"], r64["AB"])]}


def masked_active_rows(tab) -> np.ndarray:
    return np.flatnonzero(tab["mask"] == 0)


def check(got: Dict, r64: Dict, e32: Dict, tab: Dict, w: Dict, f16: bool, with_abmax: bool, ratios=None, key=None) -> List[str]:
    """Every contract of a node step a result `got` (h, AB, abmax as float64 arrays of float32 values) misses: the per-row bars,
    the exact values of masked rows, abmax = the row maxima of the AB of the same result, bit for bit."""
    bad = []
    H = r64["h"].shape[1]
    named = [("h", got["h"], r64["h"], e32["h"])] + [(f"AB{q}", g, r, e) for q, (g, r, e) in enumerate(zip(got["AB"], r64["AB"], e32["AB"]))]
    for name, g, r, e in named:
        fam = family(name, f16)
        eg = err(g, r)
        if ratios is not None:
            k = (fam,) + tuple(key)
            ratios[k] = max(ratios.get(k, 0.0), eg / max(e, YARDSTICK_FLOOR))
        if not eg <= bar(fam, e):
            d = np.abs(np.nan_to_num(g - r, nan=np.inf)).max(1) / np.maximum(np.abs(r).max(1), 1e-300)
            bad.append(f"{name}: err {eg:.3e} > {MARGINS[fam]:g} x {max(e, YARDSTICK_FLOOR):.3e} (worst row {int(d.argmax())})")
    dead = masked_active_rows(tab)
    if len(dead):
        if w["node"] is not None and np.any(got["h"][dead] != 0):
            bad.append("h' of a masked row is not exactly 0")
        for q, (W1, b1) in enumerate(w["nxt"]):
            if w["node"] is not None and (np.any(got["AB"][q][dead, :H] != _f32(b1)) or np.any(got["AB"][q][dead, H:] != 0)):
                bad.append(f"AB{q} of a masked row is not exactly [b1 | 0]")
    if with_abmax:
        for q, (ab, mx) in enumerate(zip(got["AB"], got["abmax"])):
            host = np.stack([np.abs(ab[:, :H]).max(1), np.abs(ab[:, H:]).max(1)], axis=1)
            if not np.array_equal(host, mx):
                bad.append(f"abmax{q} is not the row maxima of AB{q} (first row {int(np.flatnonzero((host != mx).any(1))[0])})")
    return bad
