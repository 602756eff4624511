"""Float64 restatement of ONE edge layer (include/hierdiff_hip.h, the comment above hd_topology_nodes / hd_edge_layer_forward).
TEST INFRASTRUCTURE ONLY.

The edge layer is the part of a GCL / EquivariantUpdate that works on edges (egnn_new.py:35-56 / :91-104 with the first Linear
factorised).  Per unmasked row (i, j) = (ei[row], ej[row]) of the topology's edge-row table (eseg[row] != 255):

    radial = |x_i - x_j|^2,  d0 = |x0_i - x0_j|^2
    pre1 = A_i + B_j + radial w_r + d0 w_d,   P = SiLU(pre1),   pre2 = W2 P + b2,   Mij = SiLU(pre2)
    GCL:    out_i += Mij sigmoid(wa.Mij + ba) / norm                (plain Mij with attention off)
    COORD:  u = (x_i - x_j) / (sqrt(radial + 1e-8) + norm_constant)
            out_i += u tanh(wa.Mij) range / norm                    (u (wa.Mij) with tanh off; fourth component 0)

`edge_layer` evaluates this graph in float64 (or, `float32=True`, the identical graph in float32 on the CPU: the yardstick the
kernels' errors are measured by) and differentiates it with torch.autograd - no hand-written backward formula.  The gradients
of the intermediate nodes are the per-row tensors the kernels materialise (csrc/k_edge_bwd.hpp):

    G2 = dL/dpre2,  P,  G1 = dL/dpre1,  escal = {dL/du (xyz), dL/dphi, dL/d(radial), dL/d(d0)}

(dL/d(radial) is the path through pre1 alone: the kernels carry the path through u as dL/du, so `u` is built from the coordinate
difference with a square root of its own.)  Rows of the table that are padding are zero in every per-row tensor.

Also here: the per-row error measure, the committed margins of tests/test_gpu_edge_layer.py, the named one-line MUTANTS of the
restatement that tests/test_edge_layer_cpu.py proves those margins reject, and the seeded inputs both tiers draw.
"""
import ctypes as C
from dataclasses import dataclass
from typing import Dict, Optional

import numpy as np
import torch
import torch.nn.functional as F

# ----------------------------------------------------------------------------- bars (EXPERIMENTS.md section AO)
# A kernel is held to `margin x the float32 CPU evaluation's own distance to float64` on the same case, per family of tensors:
#   F forward out | E per-edge G2, P, G1, escal | N node-level dAB, dx, dx0 | T per-tile partials summed on the host, G2^T P |
#   X everything in the fp16x3 training form
# Each margin is twice the worst ratio measured on an MI355X, rounded up to a power of two (table in EXPERIMENTS.md section AO); a family
# that needed more than 32 would be a finding, not a wider bar.
MARGINS = {"F": 8.0, "E": 32.0, "N": 16.0, "T": 32.0, "X": 8.0}
# A float32 result carries up to 2^-24 of relative rounding even where the float32 CPU evaluation happens to land on the float64
# value exactly (sums of one term, exact products): the yardstick is never taken below that.
YARDSTICK_FLOOR = 2.0 ** -24
FAMILY = {"out": "F", "G2": "E", "P": "E", "G1": "E", "escal_u": "E", "escal_phi": "E", "escal_rd": "E", "dAB": "N", "dx": "N",
          "dx0": "N", "dW2": "T", "db2": "T", "dwa": "T", "dba": "T", "dwrd": "T"}


def err(got, ref) -> float:
    """max over rows of max_c |got - ref| / max_c |ref| (a row = a node row, an edge row or a tile row: a tensor-wide norm hides
    one wrong row).  A row whose reference is entirely zero must be exactly zero in `got`; anything non-finite is infinitely wrong."""
    ref = np.asarray(ref, dtype=np.float64)
    ref = ref.reshape(ref.shape[0] if ref.ndim else 1, -1)
    got = np.asarray(got, dtype=np.float64).reshape(ref.shape)
    if ref.size == 0:
        return 0.0
    if not np.isfinite(got).all():
        return float("inf")
    d, s = np.abs(got - ref).max(1), np.abs(ref).max(1)
    zero = s == 0
    if (d[zero] != 0).any():
        return float("inf")
    return float((d[~zero] / s[~zero]).max()) if (~zero).any() else 0.0


def bar(family: str, err32: float, margins: Optional[Dict[str, float]] = None) -> float:
    """margins: another harness's table of families (tests/node_step_reference.py); default: MARGINS above."""
    return (MARGINS if margins is None else margins)[family] * max(err32, YARDSTICK_FLOOR)


# ----------------------------------------------------------------------------- the topology's tables (host only)
def layout(nm, em=None) -> Dict:
    """Edge-row table of a (node_mask [B, N], edge_mask [B, N, N] or None) pair from hd_topology_layout - host-only, the same
    build_layout hd_topology_create uses.  rows / tiles include the padding tiles of the last workgroup (tiles = max(1, 4 n_wg))."""
    from hierdiff_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    nm = np.ascontiguousarray(np.asarray(nm).reshape(np.asarray(nm).shape[0], -1), dtype=np.uint8)
    B, N = nm.shape
    em = None if em is None else np.ascontiguousarray(np.asarray(em).reshape(B, N, N), dtype=np.uint8)
    emp = None if em is None else em.ctypes.data
    counts = (C.c_longlong * 5)()
    _lib.check(lib.hd_topology_layout(nm.ctypes.data, emp, B, N, counts, None, None, None, None, None, None), "hd_topology_layout")
    M, E, tiles, _, rows = (int(v) for v in counts)
    ei, ej = np.zeros(rows, np.int32), np.zeros(rows, np.int32)
    eseg = np.zeros(rows, np.uint8)
    _lib.check(lib.hd_topology_layout(nm.ctypes.data, emp, B, N, counts, ei.ctypes.data, ej.ctypes.data, eseg.ctypes.data,
                                      None, None, None), "hd_topology_layout")
    active = nm.astype(bool)
    if em is not None:
        active = active | em.any(2) | em.any(1)
    node_of = np.flatnonzero(active.reshape(-1))        # compact node order: active nodes in flat order (hd_topology_nodes)
    assert len(node_of) == M
    return dict(B=B, N=N, M=M, E=E, tiles=tiles, rows=rows, ei=ei.astype(np.int64), ej=ej.astype(np.int64), eseg=eseg,
                node_of=node_of)


@dataclass
class Opts:
    """The handle's options as the edge layer sees them."""
    attention: bool = True
    tanh: bool = True
    norm_constant: float = 0.0
    coords_range: float = 30.0      # coords_range / n_layers
    norm: float = 10.0              # aggregation divisor: normalization_factor, or N for 'mean'


# ----------------------------------------------------------------------------- seeded inputs, scaled like synthetic_state_dict
def draw_inputs(M: int, H: int, seed: int, ba: bool = True) -> Dict[str, np.ndarray]:
    """Weights uniform within 1 / sqrt(fan-in) like hierdiff_amd.weights.synthetic_state_dict, node features and coordinates
    N(0, 1): pre-activations O(1).  AB = h [W1a ; W1b]^T + [b1 | 0] from an `h` and a first Linear W1 [H, 2H + 2], which are
    returned too.  float64 arrays that hold float32 values, so both arithmetics and the device see the same numbers."""
    rng = np.random.Generator(np.random.PCG64(seed))
    uni = lambda shape, fan: rng.uniform(-1.0, 1.0, shape) / np.sqrt(fan)
    h = rng.standard_normal((M, H))
    W1, b1 = uni((H, 2 * H + 2), 2 * H + 2), uni((H,), 2 * H + 2)
    x = np.pad(rng.standard_normal((M, 3)), ((0, 0), (0, 1)))
    x0 = np.pad(x[:, :3] + 0.3 * rng.standard_normal((M, 3)), ((0, 0), (0, 1)))
    d = dict(h=h, W1=W1, b1=b1, x=x, x0=x0, W2=uni((H, H), H), b2=uni((H,), H), wa=uni((H,), H),
             ba=uni((1,), H) if ba else None)
    d = {k: None if v is None else v.astype(np.float32).astype(np.float64) for k, v in d.items()}
    d["AB"] = first_linear(d["h"], d["W1"], d["b1"]).astype(np.float32).astype(np.float64)
    d["wrd"] = np.ascontiguousarray(d["W1"][:, 2 * H:].T)
    return d


def first_linear(h, W1, b1):
    """[A | B] = h [W1a ; W1b]^T + [b1 | 0]: the node-level halves of the first edge Linear (cat order [h_i, h_j, radial, d0])."""
    H = W1.shape[0]
    return np.concatenate([h @ W1[:, :H].T + b1, h @ W1[:, H:2 * H].T], axis=1)


# ----------------------------------------------------------------------------- mutants
MUTANTS = {
    "a": "the last valid row of one segment that ends in a tile's second row quad is left out of its node's sum",
    "b": "d0 taken from x instead of x0",
    "c": "ba ignored",
    "d": "1e-8 under the square root dropped",
    "e": "norm_constant dropped",
    "f": "direction x_j - x_i",
    "g": "one padding row counted as an edge of node ei[row]",
    "h": "backward only: the sending-node sum behind dB omits one node's last row",
}


def _segment_end_in_second_quad(tab) -> int:
    """Table row: valid, at offset 4..7 of its tile, and the last row of its segment."""
    eseg, rows = tab["eseg"], tab["rows"]
    for r in range(rows):
        if eseg[r] != 255 and 4 <= r % 32 < 8 and (r % 32 == 31 or eseg[r + 1] != eseg[r]):
            return r
    raise AssertionError("no segment of this batch ends in a tile's second row quad: choose another batch for mutant (a)")


# ----------------------------------------------------------------------------- the layer
def edge_layer(inp: Dict[str, np.ndarray], tab: Dict, opts: Opts, coord: bool, gouts=(), float32: bool = False,
               mutant: Optional[str] = None) -> Dict:
    """Forward and, per `gout` [M, H or 4] in `gouts`, the autograd backward.  Returns numpy float64 arrays:
    out [M, H or 4], P [rows, H], and under "bwd" one dict per gout with G2, G1 [rows, H], escal_u [rows, 3], escal_phi [rows, 1]
    (coordinate layers), escal_rd [rows, 2], dAB [M, 2H], dx, dx0 [M, 4], dW2 [H, H], db2, dwa [1, H], dwrd [2, H], dba [1, 1]
    (GCL with attention and a bias), and dW2_rows / db2_rows / dwrd_rows: the same parameter gradients as the sums a caller forms
    from the per-row tensors (G2^T P, colsum(G2), {radial, d0}^T G1)."""
    assert mutant is None or mutant in MUTANTS
    dt = torch.float32 if float32 else torch.float64
    with torch.enable_grad():
        leaf = lambda a: torch.tensor(np.asarray(a), dtype=dt, requires_grad=True)
        AB, x, x0, wrd, W2, b2, wa = (leaf(inp[k]) for k in ("AB", "x", "x0", "wrd", "W2", "b2", "wa"))
        use_ba = inp.get("ba") is not None and not coord and opts.attention
        ba = leaf(inp["ba"]) if use_ba else None
        H, M, R = W2.shape[0], AB.shape[0], tab["rows"]
        valid = np.flatnonzero(tab["eseg"] != 255)
        if mutant == "g":
            valid = np.sort(np.append(valid, np.flatnonzero(tab["eseg"] == 255)[0]))
        i, j = torch.from_numpy(tab["ei"][valid]), torch.from_numpy(tab["ej"][valid])

        diff = x[i, :3] - x[j, :3]
        if mutant == "f":
            diff = x[j, :3] - x[i, :3]
        radial = (diff ** 2).sum(1)
        y = x if mutant == "b" else x0
        d0 = ((y[i, :3] - y[j, :3]) ** 2).sum(1)
        pre1 = AB[i, :H] + AB[j, H:] + radial[:, None] * wrd[0] + d0[:, None] * wrd[1]
        P = F.silu(pre1)
        pre2 = P @ W2.T + b2
        Mij = F.silu(pre2)
        u = phi = None
        if coord:
            eps = 0.0 if mutant == "d" else 1e-8
            nc = 0.0 if mutant == "e" else opts.norm_constant
            u = diff / (torch.sqrt((diff ** 2).sum(1) + eps) + nc)[:, None]
            phi = Mij @ wa
            scal = torch.tanh(phi) * opts.coords_range if opts.tanh else phi
            msg = F.pad(u * scal[:, None], (0, 1))
        elif opts.attention:
            z = Mij @ wa
            if ba is not None and mutant != "c":
                z = z + ba
            msg = Mij * torch.sigmoid(z)[:, None]
        else:
            msg = Mij
        keep = np.ones(len(valid), dtype=bool)
        if mutant == "a":
            keep[np.searchsorted(valid, _segment_end_in_second_quad(tab))] = False
        keep_t = torch.from_numpy(keep)
        out = torch.zeros((M, msg.shape[1]), dtype=dt).index_add(0, i[keep_t], msg[keep_t]) / opts.norm

        def rows_of(t):         # per-valid-row tensor -> [table rows, width], zeros on padding rows
            t = t.detach().to(torch.float64).reshape(len(valid), -1)
            full = torch.zeros((R, t.shape[1]), dtype=torch.float64)
            full[torch.from_numpy(valid)] = t
            return full.numpy()

        res = {"out": out.detach().to(torch.float64).numpy(), "P": rows_of(P), "bwd": []}
        leaves = [AB, x, x0, wrd, W2, b2, wa] + ([ba] if ba is not None else [])
        inter = [pre2, pre1, radial, d0] + ([u, phi] if coord else [])
        for gout in gouts:
            g = torch.autograd.grad(out, leaves + inter, grad_outputs=torch.tensor(np.asarray(gout), dtype=dt), retain_graph=True,
                                    allow_unused=True)
            # (a leaf that plays no part - wa of a GCL with attention off - has gradient zero)
            g = [torch.zeros_like(v) if t is None else t.detach() for t, v in zip(g, leaves + inter)]
            nl = len(leaves)
            gAB, gx, gx0, gwrd, gW2, gb2, gwa = g[:7]
            gpre2, gpre1, grad_r, grad_d0 = g[nl:nl + 4]
            if mutant == "h":
                last = int(valid[tab["ej"][valid] == tab["ej"][valid][-1]][-1])
                pos = int(np.searchsorted(valid, last))
                gAB = gAB.clone()
                gAB[tab["ej"][last], H:] -= gpre1[pos]
            f64 = lambda t: t.to(torch.float64).numpy()
            b = {"G2": rows_of(gpre2), "G1": rows_of(gpre1), "escal_rd": rows_of(torch.stack([grad_r, grad_d0], 1)),
                 "dAB": f64(gAB), "dx": f64(gx), "dx0": f64(gx0), "dW2": f64(gW2), "db2": f64(gb2)[None], "dwa": f64(gwa)[None],
                 "dwrd": f64(gwrd)}
            if coord:
                b["escal_u"], b["escal_phi"] = rows_of(g[nl + 4]), rows_of(g[nl + 5])
            if ba is not None:
                b["dba"] = f64(g[7]).reshape(1, 1)
            # the sums a caller forms from the per-row tensors (hd_edge_layer_backward's comment), in this arithmetic
            b["dW2_rows"] = f64(gpre2.T @ P.detach())
            b["db2_rows"] = f64(gpre2.sum(0))[None]
            b["dwrd_rows"] = f64(torch.stack([radial.detach() @ gpre1, d0.detach() @ gpre1]))
            res["bwd"].append(b)
    return res
